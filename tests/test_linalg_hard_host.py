"""CPU: the inputs of tests/test_gpu_linalg_hard.py are fit for what that file asserts on the device. The builders are
imported from it, so both files see the same bits. LAPACK (through scipy) in the SAME precision solves every system: its
solution is finite and its own error measure stays under the cap the device is held to, with the observed maximum printed;
for the exact opLU cases its factorisation interchanges nothing and equals the closed form bit for bit. No device call."""
import numpy as np
import pytest
import scipy.linalg as sl

import test_gpu_linalg_hard as H

NPDS = [np.float64, np.float32]
IDS = ["f64", "f32"]


@pytest.mark.parametrize("npd", NPDS, ids=IDS)
@pytest.mark.parametrize("family", H.TRI_FAMILIES)
def test_lapack_substitution_is_finite_and_within_n_eps_on_every_triangular_case(family, npd):
    eps = float(np.finfo(npd).eps)
    top = 0.0
    sizes = [n for f, n, t in H.TRI_CASES if f == family and t is npd]
    assert sizes == [n for n in H.HARD_NS if npd is np.float64 or (family, n) not in H.F32_OVERFLOWS]
    for n in sizes:
        for upper in (False, True):
            T = H.tri_matrix(family, n, npd, upper)
            assert np.array_equal(T, np.triu(T) if upper else np.tril(T)) and (np.diag(T) != 0).all()
            assert np.array_equal(T, H.rounded(T, npd))
            for trans in (False, True):
                S, b = H.tri_problem(family, n, npd, upper, trans)
                assert np.isfinite(b).all() and np.array_equal(b, H.rounded(b, npd))
                x = H.lapack_triangular(S, b, npd, lower=(upper == trans))
                assert np.isfinite(x).all(), (family, n, upper, trans)
                w = H.omega(S, x, b)
                top = max(top, w / (n * eps))
                assert w <= n * eps, (family, n, upper, trans, w / (n * eps))
    if family == "randn":                                   # "condition number 1e14 and more" (the Float64 matrices)
        assert min(np.linalg.cond(H.tri_matrix("randn", n, np.float64, u)) for n in H.HARD_NS for u in (False, True)) >= 1e14
    print(f"LAPACK omega / (n eps), {family} {np.dtype(npd).name}: max {top:.3e}")


@pytest.mark.parametrize("family,n", H.F32_OVERFLOWS)
def test_the_float32_cases_left_out_are_those_lapack_itself_overflows_on(family, n):
    bad = 0
    for upper in (False, True):
        for trans in (False, True):
            S, b = H.tri_problem(family, n, np.float32, upper, trans)
            with np.errstate(all="ignore"):
                bad += not np.isfinite(H.lapack_triangular(S, b, np.float32, lower=(upper == trans))).all()
    assert bad >= 1


def lapack_solve(kind, A, b, npd):
    A, b = A.astype(npd), b.astype(npd)
    if kind in ("spd", "neg"):                              # -A is factored as -(L L'): LAPACK has no unpivoted L D L'
        s = -1.0 if kind == "neg" else 1.0
        return (s * sl.cho_solve(sl.cho_factor((s * A).astype(npd), lower=True, check_finite=False), b)).astype(np.float64)
    return sl.lu_solve(sl.lu_factor(A, check_finite=False), b).astype(np.float64)


@pytest.mark.parametrize("npd", NPDS, ids=IDS)
def test_lapack_is_finite_and_within_n_eps_on_every_ill_conditioned_case(npd):
    eps = float(np.finfo(npd).eps)
    top = 0.0
    for n in H.HARD_NS:
        for kind in ("spd", "neg", "gen", "gent"):
            A, b = H.ill_problem(kind, n, npd)
            assert np.isfinite(b).all() and np.array_equal(A, H.rounded(A, npd))
            if kind in ("spd", "neg"):
                assert np.array_equal(A, A.T)
                w = np.linalg.eigvalsh(A)
                assert (w > 0).all() if kind == "spd" else (w < 0).all()
            cond = np.linalg.cond(A)
            assert 0.1 * 10.0 ** H.ILL_DECADES[npd] <= cond <= 10 * 10.0 ** H.ILL_DECADES[npd], (kind, n, cond)
            x = lapack_solve(kind, A, b, npd)
            assert np.isfinite(x).all()
            e = H.eta_inf(A, x, b)
            top = max(top, e / (n * eps))
            assert e <= n * eps, (kind, n, e / (n * eps))
    print(f"LAPACK eta_inf / (n eps), ill-conditioned {np.dtype(npd).name}: max {top:.3e}")


@pytest.mark.parametrize("npd,n", H.GROWTH_CASES, ids=[f"{np.dtype(t).name}-{n}" for t, n in H.GROWTH_CASES])
def test_lapack_factors_the_growth_matrix_without_interchanges_into_the_closed_form(npd, n):
    W = H.growth_matrix(n).astype(npd)
    lu, piv = sl.lu_factor(W, check_finite=False)
    assert np.array_equal(piv, np.arange(n))
    F = H.growth_factor(n)
    assert np.isfinite(F.astype(npd)).all() and F[n - 1, n - 1] == 2.0 ** (n - 1)
    assert H.same_bits(lu, F.astype(npd))


@pytest.mark.parametrize("npd", NPDS, ids=IDS)
def test_lapack_factors_the_tied_column_without_interchanges_and_solves_within_n_eps(npd):
    n = H.TIE_N
    assert n > 1024 and 1024 <= H.TIE_LATE_ROW < n
    A = H.tie_matrix(n)
    lu, piv = sl.lu_factor(A.astype(npd), check_finite=False)
    assert np.array_equal(piv, np.arange(n))
    assert H.same_bits(lu, H.tie_factor(n).astype(npd))
    eps = float(np.finfo(npd).eps)
    for late, seed in ((None, 8800), (H.TIE_LATE_ROW, 8801)):
        A = H.tie_matrix(n, late=late)
        b = H.rounded(A @ np.random.default_rng(seed).standard_normal(n), npd)
        f = sl.lu_factor(A.astype(npd), check_finite=False)
        if late is not None:
            assert f[1][0] == late
        e = H.eta_inf(A, sl.lu_solve(f, b.astype(npd)).astype(np.float64), b)
        print(f"LAPACK eta_inf / (n eps), tie late={late} {np.dtype(npd).name}: {e / (n * eps):.3e}")
        assert e <= n * eps


@pytest.mark.parametrize("npd", NPDS, ids=IDS)
def test_the_scaling_test_stays_far_from_under_and_overflow(npd):
    """the argument of test_scaling_by_powers_of_two_commutes_bit_for_bit: entries between 1e-10 and 10, exponents in range"""
    n = 2 * H.NB + 1
    M, K, L = H.benign(n, npd)
    for A in (M, K, L[np.tril_indices(n)]):
        a = np.abs(A)
        assert 1e-10 <= a.min() and a.max() <= 10
    assert np.linalg.cond(M) <= 10 and np.linalg.cond(K) <= 10
    e, D = H.scaling(n, npd)
    assert e.min() >= -H.SCALE_EXP[npd] and e.max() <= H.SCALE_EXP[npd] and e.min() < 0 < e.max()
    assert np.array_equal(D, H.rounded(D, npd)) and np.array_equal(np.log2(D), e)
    S = M * D[:, None] * D[None, :]
    assert np.array_equal(S, H.rounded(S, npd)) and np.isfinite(S.astype(npd)).all()     # the scaled input is exact
    assert (np.linalg.inv(M) != 0).all() and (np.linalg.inv(K) != 0).all()


def test_the_non_finite_cases_sit_where_their_docstring_says():
    n, k = H.NONFINITE_N, H.NONFINITE_K
    assert n == 3 * H.NB + 1 and k // H.NB == 1 and (n - 1 - k) // H.NB == 1 and k % H.NB and (n - 1 - k) % H.NB
    L = H.benign(n, np.float64)[2]
    assert (L[np.tril_indices(n)] != 0).all() and np.linalg.cond(L) <= 10
