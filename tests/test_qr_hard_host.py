"""CPU: the inputs of tests/test_gpu_qr_hard.py are fit for what that file asserts on the device, and the NumPy models of
tests/qr_hard_cases.py are what LAPACK computes. The builders are imported from qr_hard_cases.py, so both files see the same
bits. No device call.

1. ill: LAPACK's own QR solve (gels, in the SAME precision) has eta <= 1 eps(T) in both modes on every case, tall and as the
   wide transpose; the ratios are printed (0.14 .. 0.45 eps with the seeds of ill(); no seed had to be changed). The device is
   held to 10 eps on the same operands.
2. monomial: exact_geqp3 equals LAPACK's geqp3 in permutation, rank and |diag R|; its W is the same run in Float32 and in
   Float64, and every non-zero of it is a power of two in magnitude; the T factors of the reflectors are small integers.
3. scaling: no squared column norm leaves [2^-900, 2^900], the scaled matrices are exact in the device precision, and the
   plain Householder model commutes with the scaling bit for bit.
4. non-finite: the poisoned indices of qr_hard_cases.py are a pivot position and a non-pivot position of LAPACK's
   factorisation, whose rank gap is the one test_gpu_qrp.py asserts."""
import numpy as np
import pytest
import scipy.linalg as sl

import qr_hard_cases as Q
import test_gpu_qr as tq
import test_gpu_qrp as tp
from test_gpu_linalg_hard import ILL_DECADES, SCALE_EXP, rounded, same_bits

NPDS = [np.float64, np.float32]
IDS = ["f64", "f32"]


def gels(A, b, npd, trans):
    """LAPACK's QR solve in the precision npd: min |A x - b| (trans 'N', A tall) or the minimum-norm solution of A' x = b ('T')"""
    m, n = A.shape
    f = sl.get_lapack_funcs("gels", (A.astype(npd),))
    rhs = np.zeros(max(m, n), dtype=npd)
    rhs[:len(b)] = b.astype(npd)
    _, x, info = f(np.asfortranarray(A.astype(npd)), rhs, trans=trans)
    assert info == 0
    return x[:(n if trans == "N" else m)].astype(np.float64)


@pytest.mark.parametrize("npd", NPDS, ids=IDS)
def test_lapack_qr_solve_is_within_one_eps_on_every_ill_conditioned_case(npd):
    eps = float(np.finfo(npd).eps)
    top = 0.0
    for m, n in Q.ILL_SHAPES:
        A, v, u, nA = Q.ill(m, n, npd)
        assert np.array_equal(A, rounded(A, npd)) and np.array_equal(v, rounded(v, npd)) and np.array_equal(u, rounded(u, npd))
        cond = np.linalg.cond(A)
        assert 0.1 * 10.0 ** ILL_DECADES[npd] <= cond <= 10 * 10.0 ** ILL_DECADES[npd], (m, n, cond)
        d = np.abs(np.diag(sl.qr(A.astype(npd), mode="r", pivoting=True)[0])).astype(np.float64)
        margin = d.min() / (max(m, n) * eps * d[0])             # LAPACK's geqp3 against the rank threshold rtol = max(mf, nf) eps
        print(f"LAPACK geqp3 {m}x{n} {np.dtype(npd).name}: min |R_jj| = {margin:.3g} rtol |R_11|")
        assert margin >= 2.0, (m, n, margin)                    # full rank with a factor of 2 to spare (Float64: 1e4 and more)
        At = np.ascontiguousarray(A.T)
        for tag, x, y in (("tall", gels(A, v, npd, "N"), gels(A, u, npd, "T")), ("wide", gels(At, v, npd, "T"), gels(At, u, npd, "N"))):
            e, et = Q.eta(A, nA, x, v) / eps, Q.eta(A.T, nA, y, u) / eps
            print(f"LAPACK gels {m}x{n} {tag} {np.dtype(npd).name}: eta = {e:.3f} eps, eta' = {et:.3f} eps")
            assert e <= 1.0 and et <= 1.0, (m, n, tag, e, et)
            top = max(top, e, et)
    print(f"LAPACK gels, ill-conditioned {np.dtype(npd).name}: max {top:.3f} eps")


def larft(W, taus, j0, jb):
    """T of the block column j0 .. j0 + jb by larft's recurrence, in Float64"""
    V = np.tril(np.asarray(W, dtype=np.float64)[j0:, j0:j0 + jb], -1)
    V[np.arange(jb), np.arange(jb)] = 1.0
    T = np.zeros((jb, jb))
    for c in range(jb):
        T[:c, c] = -taus[j0 + c] * (T[:c, :c] @ (V[:, :c].T @ V[:, c]))
        T[c, c] = taus[j0 + c]
    return T


@pytest.mark.parametrize("case", Q.MONOMIAL_CASES, ids=[f"{m}x{n}r{r}l{l}" for m, n, r, l in Q.MONOMIAL_CASES])
def test_exact_geqp3_is_lapack_on_every_monomial_case(case):
    mf, nf, rank, levels = case
    F = Q.monomial_case(case)
    assert F.shape == (mf, nf) and ((F != 0).sum(axis=0) == 1).all() and int((F != 0).any(axis=1).sum()) == rank
    mag = np.abs(F[F != 0])
    assert np.array_equal(np.log2(mag), np.round(np.log2(mag))) and np.abs(np.log2(mag)).max() <= levels
    assert np.linalg.matrix_rank(F) == rank
    models = {}
    for npd in NPDS:
        _, W, perm, r, taus = Q.monomial_model(case, npd)
        models[npd] = W
        assert W.dtype == npd and r == rank
        nz = np.abs(W[W != 0].astype(np.float64))
        assert np.array_equal(np.log2(nz), np.round(np.log2(nz)))                       # every non-zero is +-2^k
        assert not np.signbit(W[W == 0]).any()                                          # and every zero is +0.0
        assert set(np.unique(taus)) <= {0.0, 1.0}
        R11 = np.triu(W[:rank, :rank].astype(np.float64))
        assert np.array_equal(R11, np.diag(np.diag(R11))) and (np.diag(R11) != 0).all()  # R11 is diagonal
        _, R, lperm = sl.qr(F.astype(npd), mode="economic", pivoting=True)
        d = np.abs(np.diag(R)).astype(np.float64)
        ok = d > max(mf, nf) * float(np.finfo(npd).eps) * d[0]
        assert int(nf if ok.all() else np.argmin(ok)) == rank
        assert np.array_equal(lperm, perm), np.flatnonzero(lperm != perm)[:5]
        assert np.array_equal(d, np.abs(np.diag(W).astype(np.float64)))
        # the applies go through the compact WY form: its T factors are small integers, so with |v|, |u| <= 8 and |k| <= 2 every
        # intermediate of an apply is an integer multiple of 2^-2 far below 2^24
        tmax = max(np.abs(larft(W, taus, j0, min(Q.NB, rank - j0))).max() for j0 in range(0, rank, Q.NB))
        print(f"monomial {case} {np.dtype(npd).name}: max |T| = {tmax}")
        assert tmax <= 64
        v, u = Q.integer_rhs(case)
        x = Q.basic_solution(W, perm, rank, taus, v)
        y = Q.basic_solution_t(W, perm, rank, taus, u)
        assert np.array_equal(x, rounded(x, npd)) and np.array_equal(y, rounded(y, npd))
        assert np.array_equal(F.T @ (F @ x), F.T @ v)                                   # the normal equations hold EXACTLY
        assert np.array_equal((F.T @ y)[perm[:rank]], u[perm[:rank]])
        assert not np.signbit(x[perm[rank:]]).any() and (x[perm[rank:]] == 0).all()
    assert same_bits(models[np.float32].astype(np.float64), models[np.float64])


@pytest.mark.parametrize("npd", NPDS, ids=IDS)
def test_the_column_scaling_stays_in_range_and_commutes_with_the_model(npd):
    E = SCALE_EXP[npd]
    for m, n in Q.SCALE_SHAPES + [(65, 65)]:
        A, v, u, _ = tq.problem(m, n, npd)
        e = Q.col_exponents(n, npd)
        assert e.min() >= -E and e.max() <= E and e.min() < 0 < e.max()
        D = np.ldexp(1.0, e)
        S = A * D[None, :]
        assert np.array_equal(S, rounded(S, npd)) and np.isfinite(S.astype(npd)).all()  # the scaled input is exact
        for M in (A, S):
            sq = (M * M).sum(axis=0)
            assert 2.0 ** -900 <= sq.min() and sq.max() <= 2.0 ** 900
        Wa, ta = Q.householder_qr(A, npd)
        Ws, ts = Q.householder_qr(S, npd)
        assert same_bits(ta, ts)
        assert same_bits(np.tril(Ws, -1), np.tril(Wa, -1)) and same_bits(np.triu(Ws), np.triu(Wa) * D[None, :])
        assert same_bits(Q.qr_solve(Ws, ts, v) * D, Q.qr_solve(Wa, ta, v))
        assert same_bits(Q.qr_solve_t(Ws, ts, u), Q.qr_solve_t(Wa, ta, rounded(u / D, npd)))
        x = Q.qr_solve(Wa, ta, v)                                                       # and the model is a QR solve
        assert np.linalg.norm(x - np.linalg.lstsq(A, v, rcond=None)[0]) <= 100 * m * float(np.finfo(npd).eps) * np.linalg.norm(x)


@pytest.mark.parametrize("npd", NPDS, ids=IDS)
def test_the_uniform_scaling_is_exact_in_the_device_precision(npd):
    E = SCALE_EXP[npd]
    for shape in Q.UNIFORM_SHAPES:
        F, v, _ = tp.problem_def(*shape, npd)
        for s in (E, -E):
            S = np.ldexp(F, s)
            assert np.array_equal(np.ldexp(S, -s), F) and np.array_equal(S, rounded(S, npd))
            sq = (S * S).sum(axis=0)
            assert 2.0 ** -900 <= sq.min() and sq.max() <= 2.0 ** 900


@pytest.mark.parametrize("npd", NPDS, ids=IDS)
def test_the_non_finite_indices_sit_where_their_docstring_says(npd):
    mf, nf, r = Q.NONFINITE_SHAPE
    assert r < nf and r > Q.NB                                   # deficient, and the rank cut is past a block edge
    assert 0 <= Q.NONFINITE_PIVOT < r <= Q.NONFINITE_FREE < nf   # positions j of perm: a pivot, and one that is none
    assert 0 <= Q.NONFINITE_V < mf and 0 <= Q.NONFINITE_RES < nf
    F = tp.problem_def(*Q.NONFINITE_SHAPE, npd)[0]
    rank, _, perm, _, _ = tp.lapack_basic(F, npd)
    assert rank == r and sorted(perm.tolist()) == list(range(nf))
    X = np.linalg.pinv(F)
    assert (X != 0).all()                                        # dense: one NaN in an operand of opPinv reaches every entry
