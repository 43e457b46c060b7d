"""The cases of opLDL(M, pivot=True), shared by test_ldl_pivot_host.py (CPU) and test_gpu_ldl_pivot.py (GPU), with the host
reference: torch's CPU LAPACK (`torch.linalg.ldl_factor` / `ldl_solve`, i.e. sytrf / sytrs) in the precision under test, and a
NumPy model of the Bunch-Kaufman strategy.

Matrices. Everything is seeded with default_rng(7700 + n), drawn in the order written here, and rounded to the device
precision; v = randn(n) is drawn last.
  indef    S = (G + G') / sqrt(2 n), G = randn(n, n): 1 x 1 pivots, 1 x 1 pivots with an interchange and 2 x 2 pivots mixed.
  saddle0  q = n // 2, p = n - q, K = [0 B; B' A] with A = H H' / p + I (H = randn(p, p)) and B = randn(q, p) / sqrt(p), n >= 2: the
           unpivoted factorisation meets a zero pivot at step 1, Bunch-Kaufman takes interchanged 1 x 1 pivots only.
  pairs1   J + 1e-3 S with S as in indef; J[0, 0] = 2, J[i, i + 1] = J[i + 1, i] = 1 + i / n for i = 1, 3, 5, ... while i + 1 < n, and
           J[n - 1, n - 1] = -1 when n is even: a 2 x 2 pivot at nearly every step, and from n = 65 on one across every boundary
           between blocks of 64 (columns 63|64, 127|128, ...).

Sizes: 1, 2, 3, 5, 63, 64, 65, 77 (leading dimension 79 with NaN in the padding), 127, 128, 129, 130, 259 — panel ends, the last
single column, the 2 x 2 pivot at a panel's last column — and one Float64 run of indef and pairs1 at n = 1025 (17 panels).

Bound. eta = |M x - v|_2 / (|M|_2 |x|_2) <= 3 n eps(T): the gamma_3n of Higham, Accuracy and Stability of Numerical Algorithms,
Thm 11.3, with the growth term dropped — Bunch-Kaufman bounds it, and dropping it is what separates this from the unpivoted
test's n eps rho. Derived, not measured; test_ldl_pivot_host.py holds LAPACK itself against it."""
import functools

import numpy as np
import torch

NB = 64
NS = [1, 2, 3, 5, 63, 64, 65, 77, 127, 128, 129, 130, 259]
N_BIG = 1025
LD = {77: 79}
CASES = ("indef", "saddle0", "pairs1")
DTYPES = [torch.float64, torch.float32]
NP = {torch.float64: np.float64, torch.float32: np.float32}
ALPHA = (1.0 + np.sqrt(17.0)) / 8.0
PIVOT_NS = [5, 63, 65, 130]           # where perm and the 2 x 2 positions are held against LAPACK's (Float64, indef)


def combos():
    """(case, n) of every matrix of the suite"""
    return [(c, n) for c in CASES for n in NS if not (c == "saddle0" and n < 2)]


def _sym(rng, n):
    G = rng.standard_normal((n, n))
    return (G + G.T) / np.sqrt(2 * n)


def build(case, n, npd):
    rng = np.random.default_rng(7700 + n)
    if case == "indef":
        M = _sym(rng, n)
    elif case == "saddle0":
        q = n // 2
        p = n - q
        H = rng.standard_normal((p, p))
        A = H @ H.T / p + np.eye(p)
        B = rng.standard_normal((q, p)) / np.sqrt(p)
        M = np.block([[np.zeros((q, q)), B], [B.T, A]])
    elif case == "pairs1":
        S = _sym(rng, n)
        J = np.zeros((n, n))
        J[0, 0] = 2.0
        for i in range(1, n - 1, 2):
            J[i, i + 1] = J[i + 1, i] = 1.0 + i / n
        if n % 2 == 0:
            J[n - 1, n - 1] = -1.0
        M = J + 1e-3 * S
    else:
        raise KeyError(case)
    M = (M + M.T) / 2
    v = rng.standard_normal(n)
    return M.astype(npd).astype(np.float64), v.astype(npd).astype(np.float64)


@functools.lru_cache(maxsize=None)
def problem(case, n, npd):
    """(M, v, |M|_2, eigenvalues) in the precision the device gets, as Float64; computed once, read-only"""
    M, v = build(case, n, npd)
    w = np.linalg.eigvalsh(M)
    for a in (M, v, w):
        a.setflags(write=False)
    return M, v, float(np.abs(w).max()), w


def eta(M, norm2, x, v):
    nx = np.linalg.norm(x)
    return float(np.linalg.norm(M @ x - v) / (norm2 * nx)) if nx else float(np.linalg.norm(v))


def bound(n, dtype):
    return 3 * n * float(torch.finfo(dtype).eps)


# ------------------------------------------------------------------------------------------------ LAPACK
def lapack_solve(M, v, dtype):
    """x of M x = v by sytrf / sytrs on the CPU in `dtype`, as Float64"""
    A = torch.from_numpy(np.array(M)).to(dtype)
    LD_, piv = torch.linalg.ldl_factor(A)
    x = torch.linalg.ldl_solve(LD_, piv, torch.from_numpy(np.array(v)).to(dtype)[:, None])
    return x[:, 0].to(torch.float64).numpy()


def unroll_ipiv(ipiv):
    """LAPACK's lower-storage ipiv (1-based; a negative pair marks a 2 x 2 block whose SECOND row was interchanged) as one
    permutation, M[perm][:, perm] = L D L', and the set of first indices of the 2 x 2 blocks — what scipy.linalg.ldl does."""
    ipiv = [int(x) for x in ipiv]
    n = len(ipiv)
    perm = list(range(n))
    two = set()
    k = 0
    while k < n:
        if ipiv[k] > 0:
            p = ipiv[k] - 1
            perm[k], perm[p] = perm[p], perm[k]
            k += 1
        else:
            p = -ipiv[k] - 1
            perm[k + 1], perm[p] = perm[p], perm[k + 1]
            two.add(k)
            k += 2
    return np.array(perm), two


def lapack_pivots(M):
    A = torch.from_numpy(np.array(M))
    _, piv = torch.linalg.ldl_factor(A)
    return unroll_ipiv(piv.tolist())


# ------------------------------------------------------------------------------------------------ the NumPy model
class ZeroPivot(Exception):
    def __init__(self, info):
        super().__init__(info)
        self.info = info


def bunch_kaufman(M):
    """Unblocked Bunch-Kaufman partial pivoting in Float64 on a full symmetric copy: (perm, L, d, e) with M[perm][:, perm] =
    L D L', L unit lower and fully permuted, D = diag(d) + the sub/super-diagonal e. The four-way decision is sytf2's; the
    largest entry is the first one on a tie. Raises ZeroPivot(info) as the device does."""
    A = np.array(M, dtype=np.float64)
    n = A.shape[0]
    perm = np.arange(n)
    L, d, e = np.eye(n), np.zeros(n), np.zeros(n)
    k = 0
    while k < n:
        absakk = abs(A[k, k])
        imax, colmax = k, 0.0
        if k + 1 < n:
            col = np.abs(A[k + 1:, k])
            if np.isnan(col).any():
                raise ZeroPivot(k + 1)
            imax = k + 1 + int(np.argmax(col))
            colmax = float(col[imax - k - 1])
        if not np.isfinite(absakk) or not np.isfinite(colmax) or max(absakk, colmax) == 0.0:
            raise ZeroPivot(k + 1)
        kstep, kp = 1, k
        if absakk < ALPHA * colmax:
            row = np.abs(A[imax, k:]).copy()
            row[imax - k] = 0.0
            rowmax = float(row.max())
            with np.errstate(divide="ignore"):
                if absakk >= ALPHA * colmax * (colmax / rowmax):
                    kp = k
                elif abs(A[imax, imax]) >= ALPHA * rowmax:
                    kp = imax
                else:
                    kp, kstep = imax, 2
        kk = k + kstep - 1
        if kp != kk:
            A[[kk, kp], :] = A[[kp, kk], :]
            A[:, [kk, kp]] = A[:, [kp, kk]]
            L[[kk, kp], :k] = L[[kp, kk], :k]
            perm[[kk, kp]] = perm[[kp, kk]]
        if kstep == 1:
            d[k] = A[k, k]
            if d[k] == 0.0 or not np.isfinite(d[k]):
                raise ZeroPivot(k + 1)
            w = A[k + 1:, k].copy()
            L[k + 1:, k] = w / d[k]
            A[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], w)
        else:
            D = A[k:k + 2, k:k + 2].copy()
            det = D[0, 0] * D[1, 1] - D[0, 1] * D[1, 0]
            if det == 0.0 or not np.isfinite(det):
                raise ZeroPivot(k + 1)
            d[k], d[k + 1], e[k] = D[0, 0], D[1, 1], D[1, 0]
            Wc = A[k + 2:, k:k + 2].copy()
            Lc = Wc @ np.linalg.inv(D)
            L[k + 2:, k:k + 2] = Lc
            A[k + 2:, k + 2:] -= Lc @ Wc.T
        k += kstep
    return perm, L, d, e


def block_diag_of(d, e):
    D = np.diag(d)
    for k in np.nonzero(e)[0]:
        D[k + 1, k] = D[k, k + 1] = e[k]
    return D
