"""The inputs of the hard-input tests of the rectangular family (opQR, opQR(pivot=True), opPinv) and NumPy models of what
the device computes on them. test_qr_hard_host.py checks the inputs and the models against LAPACK on the CPU,
test_gpu_qr_hard.py runs the device; both import this module, so the two files see the same bits. Everything is seeded and
cached; the arrays are read-only Float64 arrays that hold values of the operator's element type. No device call.

ill(m, n, npd)            A = U diag(10^(-d i/(n-1))) V', d = ILL_DECADES of test_gpu_linalg_hard.py (10 / 4): condition number
                          1e10 (Float32: 1e4); v = round(A x0) is consistent, u is Gaussian (A' y = u is consistent for every u,
                          A having full column rank).
col_exponents(n, npd)     integer exponents from [-E, E], E = SCALE_EXP of test_gpu_linalg_hard.py (100 / 20).
householder_qr / qr_solve a plain unpivoted Householder QR (larfg's convention) and the two solves through it, every operation in
                          Float64 and the factor stored in npd: the model of the column-scaling test. Its sums are numpy's dots,
                          whose order depends on the length only, so a scaling by powers of two commutes with it bit for bit.
monomial(...)             one non-zero +-2^k per column: see the function. A Householder reflector of such a column is a signed
                          exchange of two rows (tau = 1, v = e_c +- e_i) or the identity (tau = 0), so every column stays
                          monomial, every intermediate is 0 or +-2^k and the factorisation is EXACT in Float32 and Float64 alike.
exact_geqp3(F, npd)       the algorithm the docstring of opQR states, step by step.
basic_solution(...)       x[perm[0:r]] = inv(R11) (Q' v)[0:r] and y = Q[:, 0:r] inv(R11') u[perm[0:r]] by substitution in Float64.
                          On a monomial factor R11 is diagonal (upper triangular with one non-zero per column and full rank), so
                          with integer v, u every intermediate is an integer times a power of two and the result is exact.
                          Zeros are +0.0: every sum of the device's applies starts from +0.0 and a sum of zeros of both signs
                          is +0.0 in round-to-nearest, so the model adds +0.0 to its result."""
import functools

import numpy as np

from test_gpu_linalg_hard import ILL_DECADES, SCALE_EXP, frozen, rounded

NB = 64
ILL_SHAPES = [(65, 64), (65, 65), (129, 65), (200, 129)]
SCALE_SHAPES = [(65, 64), (129, 65), (200, 129)]
UNIFORM_SHAPES = [(129, 65, 64), (200, 129, 65)]            # problem_def of test_gpu_qrp.py, scaled by 2^+-E
# (mf, nf, rank, levels): every step a tie of all remaining columns; a tie over more columns than the pivot search has threads
# (256); deficient with every norm exactly zero from step 257 on; the rank cut on a block edge
MONOMIAL_CASES = [(129, 65, 65, 0), (320, 300, 300, 0), (320, 300, 257, 1), (129, 65, 64, 2)]
NONFINITE_SHAPE = (200, 129, 65)
NONFINITE_V = 137            # the poisoned entry of an operand with mf entries
NONFINITE_PIVOT = 40         # j < r: u[perm[j]] is read by the transposed pivoted apply
NONFINITE_FREE = 100         # j >= r: u[perm[j]] must not be read
NONFINITE_RES = 77           # the poisoned entry of res (beta != 0)


# ------------------------------------------------------------------------------------------------ ill-conditioned
@functools.lru_cache(maxsize=None)
def ill(m, n, npd):
    """(A, v, u, |A|_2): A = U diag(10^(-d i/(n-1))) V' rounded to npd, v = round(A x0), u Gaussian; seed 9800 + 7 m + n"""
    rng = np.random.default_rng(9800 + 7 * m + n)
    U = np.linalg.qr(rng.standard_normal((m, n)))[0]
    V = np.linalg.qr(rng.standard_normal((n, n)))[0]
    s = 10.0 ** (-ILL_DECADES[npd] * np.arange(n) / max(n - 1, 1))
    A = rounded((U * s) @ V.T, npd)
    v = rounded(A @ rng.standard_normal(n), npd)
    u = rounded(rng.standard_normal(n), npd)
    frozen(A, v, u)
    return A, v, u, float(np.linalg.norm(A, 2))


def eta(A, nA, x, v):
    """|v - A x| / (|A| |x| + |v|): the normwise backward error of x as a solution of the consistent system A x = v"""
    return float(np.linalg.norm(v - A @ x) / (nA * np.linalg.norm(x) + np.linalg.norm(v)))


# ------------------------------------------------------------------------------------------------ powers of two
@functools.lru_cache(maxsize=None)
def col_exponents(n, npd):
    """n integer exponents from [-E, E], E = SCALE_EXP[npd]; seed 9850 + n"""
    e = np.random.default_rng(9850 + n).integers(-SCALE_EXP[npd], SCALE_EXP[npd] + 1, n)
    return frozen(e)[0]


def larfg(x):
    """(beta, tau, scale) of the reflector of x in larfg's convention: beta = -sign(alpha) |x|, tau = (beta - alpha) / beta,
    v = x[1:] scale with scale = 1 / (alpha - beta); x[1:] == 0: tau = 0, H = I, beta = alpha"""
    alpha, sigma = float(x[0]), float(x[1:] @ x[1:])
    if sigma == 0.0:
        return alpha, 0.0, 0.0
    beta = -float(np.copysign(np.sqrt(alpha * alpha + sigma), alpha))
    return beta, (beta - alpha) / beta, 1.0 / (alpha - beta)


def householder_qr(A, npd):
    """(W, taus): unpivoted Householder QR of the tall A, W in LAPACK's layout with its entries rounded to npd after every step"""
    W = np.array(A, dtype=np.float64)
    m, n = W.shape
    taus = np.zeros(n)
    for c in range(n):
        beta, tau, scale = larfg(W[c:, c])
        v = np.concatenate([[1.0], rounded(W[c + 1:, c] * scale, npd)])
        if tau != 0.0 and c + 1 < n:
            C = W[c:, c + 1:]
            W[c:, c + 1:] = rounded(C - np.outer(v, tau * (v @ C)), npd)
        W[c, c] = rounded(beta, npd)
        W[c + 1:, c] = v[1:]
        taus[c] = tau
    return W, taus


def reflect(W, taus, r, z, reverse=False):
    """Q' z for the leading r reflectors of W (reverse: Q z), in Float64"""
    z = np.array(z, dtype=np.float64)
    for c in (reversed(range(r)) if reverse else range(r)):
        if taus[c] != 0.0:
            v = np.concatenate([[1.0], W[c + 1:, c]])
            z[c:] -= v * (taus[c] * (v @ z[c:]))
    return z


def back_substitute(R, b):
    x = np.array(b, dtype=np.float64)
    for j in reversed(range(len(x))):
        x[j] = (x[j] - R[j, j + 1:] @ x[j + 1:]) / R[j, j]
    return x


def forward_substitute_t(R, b):
    """the solution of R' x = b"""
    x = np.array(b, dtype=np.float64)
    for j in range(len(x)):
        x[j] = (x[j] - R[:j, j] @ x[:j]) / R[j, j]
    return x


def qr_solve(W, taus, v):
    """x = inv(R) (Q' v)[0:n]"""
    n = W.shape[1]
    return back_substitute(W[:n, :], reflect(W, taus, n, v)[:n])


def qr_solve_t(W, taus, u):
    """y = Q [inv(R') u; 0]"""
    m, n = W.shape
    return reflect(W, taus, n, np.concatenate([forward_substitute_t(W[:n, :], u), np.zeros(m - n)]), reverse=True)


# ------------------------------------------------------------------------------------------------ monomial matrices
@functools.lru_cache(maxsize=None)
def monomial(m, n, nrows, levels, seed):
    """m x n, one non-zero +-2^k per column with |k| <= levels. The non-zeros sit in nrows distinct rows: the first nrows columns
    take one row each, the others share those rows at random; the columns are then shuffled. The rank is exactly nrows."""
    rng = np.random.default_rng(seed)
    rows = rng.choice(m, size=nrows, replace=False)
    owner = np.concatenate([np.arange(nrows), rng.integers(nrows, size=n - nrows)])
    vals = rng.choice([-1.0, 1.0], size=n) * np.ldexp(1.0, rng.integers(-levels, levels + 1, n))
    F = np.zeros((m, n))
    F[rows[owner], np.arange(n)] = vals
    F = np.ascontiguousarray(F[:, rng.permutation(n)])
    return frozen(F)[0]


def monomial_case(case):
    mf, nf, rank, levels = case
    return monomial(mf, nf, rank, levels, 9900 + 7 * mf + nf + rank + levels)


def exact_geqp3(F, npd, rtol=None):
    """(W, perm, rank, taus): at step c the squared norms of the remaining columns over the rows c and below, in Float64; the
    pivot is the FIRST largest one in the current memory order; the columns are exchanged; the larfg reflector of the pivot
    column (x == 0: tau = 0) is applied to the columns behind it. W in LAPACK's layout with its entries of type npd, F[:, perm[j]]
    is column j of Q R, rank = the length of the leading run of j with |R_jj| > rtol |R_11| (default max(m, n) eps(npd))."""
    W = np.array(F, dtype=npd)
    m, n = W.shape
    perm = np.arange(n)
    taus = np.zeros(n)
    for c in range(n):
        sub = W[c:, c:].astype(np.float64)
        p = c + int(np.argmax((sub * sub).sum(axis=0)))                   # argmax: the first of the largest
        if p != c:
            W[:, [c, p]] = W[:, [p, c]]
            perm[[c, p]] = perm[[p, c]]
        x = W[c:, c].astype(np.float64)
        beta, tau, scale = larfg(x)
        v = np.concatenate([[1.0], (x[1:] * scale).astype(npd).astype(np.float64)])
        if tau != 0.0 and c + 1 < n:
            C = W[c:, c + 1:].astype(np.float64)
            W[c:, c + 1:] = (C - np.outer(v, tau * (v @ C))).astype(npd)
        W[c, c] = beta
        W[c + 1:, c] = v[1:]
        taus[c] = tau
    d = np.abs(np.diag(W).astype(np.float64))
    rtol = max(m, n) * float(np.finfo(npd).eps) if rtol is None else rtol
    ok = d > rtol * d[0]
    return W, perm, int(n if ok.all() else np.argmin(ok)), taus


def basic_solution(W, perm, rank, taus, v):
    """x with x[perm[0:r]] = inv(R11) (Q' v)[0:r] and +0.0 elsewhere"""
    W = np.asarray(W, dtype=np.float64)
    x = np.zeros(W.shape[1])
    x[perm[:rank]] = back_substitute(W[:rank, :rank], reflect(W, taus, rank, v)[:rank])
    return x + 0.0


def basic_solution_t(W, perm, rank, taus, u):
    """y = Q[:, 0:r] inv(R11') u[perm[0:r]]"""
    W = np.asarray(W, dtype=np.float64)
    w = forward_substitute_t(W[:rank, :rank], np.asarray(u, dtype=np.float64)[perm[:rank]])
    return reflect(W, taus, rank, np.concatenate([w, np.zeros(W.shape[0] - rank)]), reverse=True) + 0.0


@functools.lru_cache(maxsize=None)
def monomial_model(case, npd):
    """(F, W, perm, rank, taus) of a monomial case, factored once"""
    F = monomial_case(case)
    W, perm, rank, taus = exact_geqp3(F, npd)
    frozen(W, perm, taus)
    return F, W, perm, rank, taus


@functools.lru_cache(maxsize=None)
def integer_rhs(case):
    """(v, u): mf and nf integers from [-8, 8]"""
    mf, nf = case[:2]
    rng = np.random.default_rng(9950 + 7 * mf + nf + case[2])
    return frozen(rng.integers(-8, 9, mf).astype(np.float64), rng.integers(-8, 9, nf).astype(np.float64))
