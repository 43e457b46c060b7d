"""Random cases for the factorisation operators (opCholesky, opLDL, opLU, triangular opInverse, opQR with and without pivot=True,
opPinv): the generator that tests/test_linalg_fuzz_host.py (CPU) and tests/test_gpu_linalg_fuzz.py (-m gpu) share, so that both
see the same cases. `case(seed)` is plain numpy data, a function of default_rng(88000 + seed) alone; nothing is rejected or
redrawn. The matrices are the well-conditioned families of the pinned test files, imported: they are functions of the shape,
so two seeds that draw the same shape share a matrix and differ in storage, operand, wrapper and scalars.

What is drawn (every draw is made for every seed, in a fixed order, whether or not the case uses it):
  family    chol, ldl, lu, lower, upper, qr, qrp, pinv; the first 2 len(FORCED) seeds take family and shape from FORCED instead
  dtype     Float64 for even seeds, Float32 for odd ones
  size      n (square) or nf: a third each 8 .. 16, 64 j + d (j in 1 .. 4, d in -1, 0, 1), 8 .. 259
            mf = nf + (0 a third of the time, else 1 .. 299); rank 1 .. nf - 1, one draw in five full rank; tall or wide
  storage   col (column-major, ld = rows + 0 .. 3), row (row-major, the same padding), offset (either, starting 1 .. 3 elements
            into the allocation), strided (big[::2, ::2], which the constructors copy); NaN in every element that is not the matrix
  operand   a vector, or a matrix of k = 2 .. 17 columns (one in eight: 24); ldv, ldr = rows + 0 .. 3 independently; element
            offset 0 .. 3; 64 sentinel elements in front and behind (NaN for V, 7.25 for res, so that a read-modify-write shows)
  wrapper   op, transpose(op), adjoint(op)
  scalars   the 3-argument form, (1, 0), (2, 0) on a NaN-filled res, (0.75, -1.25), (-1, 1)
  refine    0, 0, 0, 1, 2 for chol, ldl, lu
  rtol      for qrp and pinv sqrt(eps(T)); None (the default max(mf, nf) eps) in half of the cases with max(mf, nf) >= 96
  alias     square families: one case in four also runs mul!(x, op, x)

The right-hand sides are Gaussian, except in the minimum-norm mode of qrp, whose basic solution solves consistent systems
only: there U = F' W, rounded. `ratios(c, X)` is observed / bound of the family's metrics for a result X, with the functions
and bounds of the family's pinned test file."""
import functools
import os
import types

import numpy as np

import test_gpu_ldl as t_ldl
import test_gpu_linalg as t_chol
import test_gpu_lu as t_lu
import test_gpu_pinv as t_pinv
import test_gpu_qr as t_qr
import test_gpu_qrp as t_qrp

BASE_SEED = 88000
DEFAULT_SEEDS = 320
SQUARE = ("chol", "ldl", "lu", "lower", "upper")
RECT = ("qr", "qrp", "pinv")
FAMILIES = SQUARE + RECT
REFINABLE = ("chol", "ldl", "lu")
STORAGES = ("col", "row", "offset", "strided")
WRAPPERS = ("op", "transpose", "adjoint")
SCALARS = (None, (1.0, 0.0), (2.0, 0.0), (0.75, -1.25), (-1.0, 1.0))
NAN_RES = 2                                     # the index in SCALARS whose res is NaN-filled
REFINES = (0, 0, 0, 1, 2)
GUARD = 64
RES_SENTINEL = 7.25
# each entry runs once per precision: seeds 2 i and 2 i + 1
FORCED = ([(f, n) for n in (128, 192, 256) for f in SQUARE]
          + [("qr", (128, 128)), ("qr", (192, 128)), ("qr", (256, 192)), ("qr", (32833, 65))]
          + [(f, s) for f in ("qrp", "pinv") for s in ((128, 128, 64), (192, 128, 127), (40001, 65, 64))])
BIG_ROWS = 600                                  # no drawn case has more rows; the forced ones above it are timed


def seeds():
    """the seeds of a run: 0 .. MXLO_LINFUZZ_SEEDS - 1, so a larger value only extends the list"""
    return range(int(os.environ.get("MXLO_LINFUZZ_SEEDS", str(DEFAULT_SEEDS))))


def rounded(a, npd):
    return np.asarray(a).astype(npd).astype(np.float64)


def draw_size(rng):
    which = int(rng.integers(3))
    small, j, d, wide = int(rng.integers(8, 17)), int(rng.integers(1, 5)), int(rng.integers(-1, 2)), int(rng.integers(8, 260))
    return (small, 64 * j + d, wide)[which]


@functools.lru_cache(maxsize=None)
def matrix(family, shape, npd):
    """(the tall or square matrix of the family at this shape, rounded to npd, as Float64; its norm for the metric; rho)"""
    if family in ("chol", "lower", "upper"):
        M, L, nM, _ = t_chol.problem(shape, npd)
        if family == "chol":
            return M, nM, 1.0
        return (L if family == "lower" else np.ascontiguousarray(L.T)), float(np.sqrt(nM)), 1.0
    if family == "ldl":
        K, _, nK, _, _, _, rho = t_ldl.problem(shape, npd)
        return K, nK, rho
    if family == "lu":
        A, _, nA = t_lu.problem(shape, npd)
        return A, nA, 1.0
    if family == "qr":
        A, _, _, nA = t_qr.problem(*shape, npd)
        return A, nA, 1.0
    F, _, nF = t_qrp.problem_def(*shape, npd)
    return F, nF, 1.0


def case(seed):
    rng = np.random.default_rng(BASE_SEED + seed)
    npd = np.float64 if seed % 2 == 0 else np.float32
    eps = float(np.finfo(npd).eps)
    c = types.SimpleNamespace(seed=seed, npd=npd, eps=eps, forced=seed < 2 * len(FORCED))
    # ---- every draw, in a fixed order
    family = FAMILIES[int(rng.integers(len(FAMILIES)))]
    n = draw_size(rng)
    extra = 0 if rng.integers(3) == 0 else int(rng.integers(1, 300))
    full_rank = rng.integers(5) == 0
    rank_draw = float(rng.random())
    wide = bool(rng.integers(2))
    storage = STORAGES[int(rng.integers(4))]
    pad, off, offset_rowmajor = int(rng.integers(0, 4)), int(rng.integers(1, 4)), bool(rng.integers(2))
    vector = rng.integers(2) == 0
    k = int(rng.integers(2, 18))
    if rng.integers(8) == 0:
        k = 24
    padv, padr, offv, offr = (int(x) for x in rng.integers(0, 4, size=4))
    c.wrapper = WRAPPERS[int(rng.integers(3))]
    c.scalars_index = int(rng.integers(len(SCALARS)))
    refine = REFINES[int(rng.integers(len(REFINES)))]
    default_rtol = bool(rng.integers(2))
    alias = rng.integers(4) == 0
    # ---- family and shape
    if c.forced:
        family, shape = FORCED[seed // 2]
    elif family in SQUARE:
        shape = n
    elif family == "qr":
        shape = (n + extra, n)
    else:
        shape = (n + extra, n, n if full_rank else 1 + min(n - 2, int(rank_draw * (n - 1))))
    c.family, c.shape = family, shape
    c.square = family in SQUARE
    c.F, c.norm, c.rho = matrix(family, shape, npd)
    c.mf, c.nf = c.F.shape
    c.rank = shape[2] if family in ("qrp", "pinv") else c.nf
    c.wide = wide and c.mf > c.nf                           # a square matrix is its own tall orientation
    c.A = c.F.T if c.wide else c.F                          # what the constructor gets
    c.refine = refine if family in REFINABLE else 0
    c.rtol = None
    if family in ("qrp", "pinv") and not (default_rtol and max(c.mf, c.nf) >= 96):
        c.rtol = float(np.sqrt(eps))
    c.rtol_value = max(c.mf, c.nf) * eps if c.rtol is None else c.rtol
    # ---- storage of the matrix
    c.storage = storage
    c.rowmajor = offset_rowmajor if storage == "offset" else storage == "row"
    c.pad, c.off = pad, (off if storage == "offset" else 0)
    # ---- the apply: lsq takes mf entries to nf, the minimum-norm mode nf to mf; a square family takes n to n
    c.transposed = c.wrapper != "op"
    c.lsq = c.square or (c.transposed == c.wide)
    c.rows_in, c.rows_out = (c.mf, c.nf) if c.lsq else (c.nf, c.mf)
    c.k = 1 if vector else k
    c.vector = bool(vector)
    c.ldv, c.ldr, c.offv, c.offr = c.rows_in + padv, c.rows_out + padr, offv, offr
    c.scalars = SCALARS[c.scalars_index]
    c.alias = bool(alias) and c.square
    if family == "qrp" and not c.lsq:
        c.V = rounded(c.F.T @ rng.standard_normal((c.mf, c.k)), npd)
    else:
        c.V = rounded(rng.standard_normal((c.rows_in, c.k)), npd)
    c.res0 = rounded(rng.standard_normal((c.rows_out, c.k)), npd)
    if c.scalars_index == NAN_RES:
        c.res0 = np.full_like(c.res0, np.nan)
    return c


def op_key(c):
    """cases with the same key may share one operator"""
    return (c.family, c.shape, c.wide, c.npd, c.storage, c.rowmajor, c.pad, c.off, c.refine, c.rtol)


def matrix_storage(c):
    """(flat buffer in the case's precision, shape, strides, offset — in elements) of c.A in its drawn storage; every element
    that is not the matrix holds NaN"""
    rows, cols = c.A.shape
    if c.storage == "strided":
        ld = 2 * rows + c.pad
        buf = np.full(ld * 2 * cols, np.nan, dtype=c.npd)
        strides, offset = (2, 2 * ld), 0
    else:
        ld = (cols if c.rowmajor else rows) + c.pad
        buf = np.full(c.off + ld * (rows if c.rowmajor else cols) + 4, np.nan, dtype=c.npd)
        strides, offset = ((ld, 1) if c.rowmajor else (1, ld)), c.off
    window(buf, (rows, cols), strides, offset)[...] = c.A
    return buf, (rows, cols), strides, offset


def operand_storage(X, ld, off, sentinel):
    """(flat buffer, shape, strides, offset) of the column-major operand X in leading dimension ld, `off` elements behind a
    guard zone, another guard zone behind it; padding and guards hold `sentinel`. A vector case has one column and is viewed
    with the shape (rows,)."""
    rows, k = X.shape
    buf = np.full(GUARD + off + ld * k + GUARD, sentinel, dtype=X.dtype)
    window(buf, (rows, k), (1, ld), GUARD + off)[...] = X
    return buf, (rows, k), (1, ld), GUARD + off


def window(buf, shape, strides, offset):
    item = buf.itemsize
    return np.lib.stride_tricks.as_strided(buf[offset:], shape, tuple(s * item for s in strides))


def outside(buf, shape, strides, offset):
    """the elements of buf that are not in the window, as raw bits"""
    mask = np.ones(buf.shape, dtype=bool)
    window(mask, shape, strides, offset)[...] = False
    return buf.view(np.uint64 if buf.itemsize == 8 else np.uint32)[mask]


@functools.lru_cache(maxsize=None)
def full_rank_range_basis(shape, npd):
    """an orthonormal basis of range(A) for the full-rank A of the qr family, from a Float64 Householder QR. (The left singular
    vectors that test_gpu_qrp.range_basis takes, which a rank-deficient matrix needs, carry a few eps more of their own: LAPACK's
    minimum-norm solution at 11 x 9 measures 0.64 of the bound 11 eps against them and 0.25 against this basis.)"""
    return np.linalg.qr(matrix("qr", shape, npd)[0])[0]


def system_matrix(c):
    """the matrix whose solve the drawn wrapper is, for the square families: c.F or its transpose"""
    return c.F.T if c.transposed else c.F


def ratios(c, X):
    """observed / bound per metric of the family for the result X (rows_out x k, Float64) of the plain apply to c.V: the worst
    column. The bounds are n eps(T) (chol, lower, upper in the 2-norm; lu in the infinity norm), n eps(T) rho (ldl) and
    mf eps(T) (qr, qrp, pinv), with the metric functions of the family's pinned test file."""
    out = {}

    def put(name, value, bound):
        out[name] = max(out.get(name, 0.0), value / bound)

    F, nF = c.F, c.norm
    bound = c.mf * c.eps
    # the distance from range(F) is taken for mf > nf only. For a square full-rank F the range is the whole space and the number
    # measures nothing; for a square rank-deficient F of 8 .. 16 rows the bound is 8 .. 16 eps, and the host's own basis (left
    # singular vectors) and LAPACK's solution together fill up to 0.77 of it in Float64 (seeds 1370, 2402, 3724 of 4000)
    proper_range = c.mf > c.nf
    for j in range(c.k):
        x, v = X[:, j], c.V[:, j]
        if c.family in ("chol", "lower", "upper"):
            put("eta", t_chol.eta(system_matrix(c), nF, x, v), bound)
        elif c.family == "ldl":
            put("eta", t_ldl.eta(F, nF, x, v), bound * c.rho)
        elif c.family == "lu":
            At = system_matrix(c)
            put("eta_inf", t_lu.eta_inf(At, t_lu.norm_inf(At), x, v), bound)
        elif c.family == "qr" and c.lsq:
            put("lsq", t_qr.lsq_error(F, nF, v, x), bound)
        elif c.family == "qr":
            put("minnorm residual", t_qr.minimum_norm_residual(F, nF, v, x), bound)
            if c.mf > c.nf:
                B = full_rank_range_basis(c.shape, c.npd)
                put("minnorm range", float(np.linalg.norm(x - B @ (B.T @ x)) / np.linalg.norm(x)), bound)
        elif c.family == "qrp" and c.lsq:
            put("lsq", t_qrp.lsq_error(F, nF, v, x), bound)
        elif c.family == "qrp":
            res, dist = t_qrp.wide_errors(F, nF, v, x)
            put("wide residual", res, bound)
            if proper_range:
                put("wide range", dist, bound)
        elif c.lsq:
            put("lsq x", t_qrp.lsq_error(F, nF, v, x), bound)
            if c.rank < c.nf:
                put("row space x", t_pinv.space_distance(F.T, x), bound)
        else:
            put("lsq y", t_qrp.lsq_error(F.T, nF, v, x), bound)
            if proper_range:
                put("range y", t_pinv.space_distance(F, x), bound)
    return out
