"""The inputs of the iterative-refinement tests (`refine=r` of opCholesky, opLDL, opLU) and a NumPy model of the scheme.
test_refine_host.py runs the model on them on the CPU, test_gpu_refine.py the device; both import this module, so the
two files see the same matrices, step counts and bounds. Everything is seeded and cached; the arrays are read-only
Float64 arrays that hold values of the operator's element type."""
import functools

import numpy as np

NB = 64
SIZES = [1, 5, 63, 64, 65, 77, 129, 257]        # 77 lives in a leading dimension of 79 with NaN padding on the device
LD = {77: 79}
BIG = 2049                                      # Float64, the hard LDL' family only
DELTA = {np.float64: 1e-6, np.float32: 1e-2}
# (element type, refine) of the hard LDL' family
LDL_CASES = [(np.float64, 1), (np.float64, 2), (np.float32, 2)]
F32_STEPS = 2                                   # the Float32 forward-error family
WELL_SIZES = [65, 129]                          # the well-conditioned family, Float64, refine = 1


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def hard_ldl(n, npd):
    """(K, v): K = (G + G')/2, G = randn(n, n)/sqrt(n) from default_rng(7300 + n), every third diagonal entry replaced by
    delta (1 + 0.5 u): small pivots inside every block of 64 and across block edges, which an unpivoted LDL' takes as
    they come. v is drawn after G and the u."""
    rng = np.random.default_rng(7300 + n)
    G = rng.standard_normal((n, n)) / np.sqrt(n)
    K = (G + G.T) / 2
    for i in range(0, n, 3):
        K[i, i] = DELTA[npd] * (1 + 0.5 * rng.random())
    v = rng.standard_normal(n)
    return _ro(K.astype(npd).astype(np.float64), v.astype(npd).astype(np.float64))


@functools.lru_cache(maxsize=None)
def cond1e4(n, kind):
    """(A, v) in Float32 with cond_2 = 1e4: kind "spd": Q diag(s) Q', "gen": Q diag(s) P', s = logspace(0, -4, n), Q and P
    from the QR of default_rng(8100 + n) normals."""
    rng = np.random.default_rng(8100 + n)
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    P = np.linalg.qr(rng.standard_normal((n, n)))[0]
    s = np.logspace(0, -4, n)
    v = rng.standard_normal(n)
    if kind == "spd":
        A = (Q * s) @ Q.T
        A = (A + A.T) / 2                                   # exactly symmetric before and so after the rounding
    else:
        A = (Q * s) @ P.T
    return _ro(A.astype(np.float32).astype(np.float64), v.astype(np.float32).astype(np.float64))


def simple_matrix(rng, n):
    """test/test_aux.jl:3-17 for a real element type: U S V' with singular values 1 .. 2"""
    U = np.linalg.qr(rng.random((n, n)))[0]
    V = np.linalg.qr(rng.random((n, n)))[0]
    return U @ np.diag(1 + np.arange(n) / max(n - 1, 1)) @ V.T


@functools.lru_cache(maxsize=None)
def well(base, n):
    """(A, v), Float64: the well-conditioned matrices of the factorisation tests. H = G G' + I (opCholesky); H with the sign
    flipped where row and column index are both 2 mod 3, quasi-definite (opLDL); H with its rows rolled down by NB + 1
    (opLU); simple_matrix (opLU)."""
    rng = np.random.default_rng(5200 + n)
    G = rng.standard_normal((n, n)) / np.sqrt(n)
    H = G @ G.T + np.eye(n)
    H = (H + H.T) / 2
    if base == "chol":
        A = H
    elif base == "ldl":
        s = np.arange(n) % 3 == 2
        A = np.where(s[:, None] & s[None, :], -H, H)
    elif base == "lu":
        A = np.roll(H, NB + 1, axis=0)
    else:
        A = simple_matrix(np.random.default_rng(6200 + n), n)
    v = np.random.default_rng(7200 + n).standard_normal(n)
    return _ro(np.array(A, dtype=np.float64), v)


# ------------------------------------------------------------------------------------------------ measures
_NORMS = {}


def norm2(A):
    """|A|_2, computed once per (cached, read-only) matrix"""
    if id(A) not in _NORMS:
        sym = np.array_equal(A, A.T)
        _NORMS[id(A)] = (A, float(np.abs(np.linalg.eigvalsh(A)).max() if sym else np.linalg.norm(A, 2)))
    return _NORMS[id(A)][1]


def eta2(A, x, v):
    """|A x - v|_2 / (|A|_2 |x|_2), the normwise backward error of x"""
    return float(np.linalg.norm(A @ x - v) / (norm2(A) * np.linalg.norm(x)))


def eta_inf(A, x, v):
    """the measure of the factorisation tests: |A x - v|_inf / (|A|_inf |x|_inf)"""
    return float(np.abs(A @ x - v).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max()))


def forward_error(x, xs):
    return float(np.abs(x - xs).max() / np.abs(xs).max())


# ------------------------------------------------------------------------------------------------ the model
# Every operation below is an elementwise or BLAS operation on arrays of the precision npd, so Float32 is computed in
# Float32 (numpy.linalg's own solvers compute Float32 problems in double and would be too kind a model).
def _tri_solve(Tm, b, lower, unit=False):
    """column-oriented substitution with a triangular matrix, in Tm's precision"""
    n = Tm.shape[0]
    x = b.astype(Tm.dtype).copy()
    for p in (range(n) if lower else range(n - 1, -1, -1)):
        if not unit:
            x[p] /= Tm[p, p]
        if lower:
            x[p + 1:] -= Tm[p + 1:, p] * x[p]
        else:
            x[:p] -= Tm[:p, p] * x[p]
    return x


def _factor_sym(K, npd, ldl):
    """the lower triangle of the UNPIVOTED L D L' (unit L below the diagonal, d on it) or of the Cholesky factor of K,
    right-looking in blocks of NB"""
    A = K.astype(npd).copy()
    n = A.shape[0]
    for j0 in range(0, n, NB):
        j1 = min(n, j0 + NB)
        for p in range(j0, j1):
            if not ldl:
                A[p, p] = np.sqrt(A[p, p])
            A[p + 1:, p] /= A[p, p]
            if p + 1 < j1:
                A[p + 1:, p + 1:j1] -= np.outer(A[p + 1:, p], (A[p, p] if ldl else npd(1)) * A[p + 1:j1, p])
        if j1 < n:
            P = A[j1:, j0:j1]
            A[j1:, j1:] -= ((P * np.diag(A)[j0:j1]) if ldl else P) @ P.T
    return A


def ldl_solver(K, npd):
    """F \\ b for the UNPIVOTED L D L' of K, factored and solved in precision npd"""
    A = _factor_sym(K, npd, True)
    d = np.diag(A).copy()
    L, Lt = np.tril(A), np.ascontiguousarray(np.tril(A).T)
    return lambda b: _tri_solve(Lt, _tri_solve(L, b, True, unit=True) / d, False, unit=True)


def chol_solver(A, npd):
    L = np.tril(_factor_sym(A, npd, False))
    Lt = np.ascontiguousarray(L.T)
    return lambda b: _tri_solve(Lt, _tri_solve(L, b, True), False)


def lu_solver(A, npd, trans=False):
    """F \\ b (trans: F' \\ b) for the partially pivoted LU of A, factored and solved in precision npd"""
    W = A.astype(npd).copy()
    n = W.shape[0]
    perm = np.arange(n)
    for p in range(n):
        r = p + int(np.argmax(np.abs(W[p:, p])))
        if r != p:
            W[[p, r]] = W[[r, p]]
            perm[[p, r]] = perm[[r, p]]
        W[p + 1:, p] /= W[p, p]
        W[p + 1:, p + 1:] -= np.outer(W[p + 1:, p], W[p, p + 1:])
    Wt = np.ascontiguousarray(W.T)

    def solve(b):
        b = b.astype(npd)
        if not trans:
            return _tri_solve(W, _tri_solve(W, b[perm], True, unit=True), False)
        x = np.empty(n, dtype=npd)
        x[perm] = _tri_solve(Wt, _tri_solve(Wt, b, True), False, unit=True)
        return x
    return solve


def refine_model(A, v, solve, steps, npd):
    """x_0 = F \\ v, then `steps` times x += F \\ (v - A x): factor and solve in npd, residual and x in Float64, one rounding"""
    x = solve(v).astype(np.float64)
    for _ in range(steps):
        r = v - A @ x
        x = x + solve(r).astype(np.float64)
    return x.astype(npd).astype(np.float64)
