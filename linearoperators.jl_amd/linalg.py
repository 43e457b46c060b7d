"""opCholesky, opLDL, opLU and triangular opInverse — src/linalg.jl:3-9 (mulFact!), :27-32 (opInverse), :44-58 (opCholesky),
:60-75 with ext/LinearOperatorsLDLFactorizationsExt.jl:5-18 (opLDL of a dense matrix).

The factorisation, the inverses of the diagonal blocks and the block substitution sweeps run in libmxlo.so
(csrc/linalg.hip); this module is the host mirror: argument checks, the storage an operator owns, the closures.
Real Float64 / Float32 only. `mul!` on an n x k matrix (`F \\ V`, src/operations.jl:34-36) takes the block form of the sweeps for k > 1
(`mxlo_*_mul_block`): the chain of launches of one vector apply and one read of the factor per GROUP = 8 columns, each column
bit-identical to its vector apply. The inverse of a general dense matrix is `opLU` (partially pivoted LU); `opInverse` itself
stays triangular-only. `opLDL(M, pivot=True)` is the Bunch–Kaufman form Pᵀ M P = L D Lᵀ with 1 x 1 and 2 x 2 pivots (`mxlo_sytrf`,
`mxlo_ldlp_mul`, `mxlo_ldlp_mul_block`), `ldl_inertia` the inertia it reveals; a sparse LDLᵀ is not provided. `refine=r` on the three
factorisation operators adds r steps of iterative refinement to every apply (`mxlo_*_mul_refine`), with the residual and the
iterate in Float64 and a snapshot of M the operator keeps. `opQR` is the rectangular `M \\ v`: least-squares and minimum-norm
solves through an unpivoted Householder QR (`mxlo_geqrf`, `mxlo_qr_mul`, and `mxlo_qr_mul_block` for matrix operands), or — `pivot=True` —
through a column-pivoted, rank-revealing one (`mxlo_geqp3`, `mxlo_qrp_mul`, `mxlo_qrp_mul_block`). `opPinv` is the pseudo-inverse of a
matrix of any rank: the pivoted QR completed to an orthogonal decomposition (`mxlo_cod_factor`, `mxlo_pinv_mul`, `mxlo_pinv_mul_block`).
"""
from __future__ import annotations

import ctypes as C
import numbers

import torch

from . import _lib
from .device import Storage, ctx_of, dtype_code, get_ctx
from .leaves import _stored_colmajor
from .operators import LinearOperator, LinearOperatorException, columnwise, state_version

BLOCK = 64            # block column width of csrc/linalg.hip (NB)
GROUP = 8             # right-hand sides per pass of the block sweeps (KB): the work matrix is n x GROUP doubles
MAX_REFINE = 8        # largest `refine`: only there to stop a typo from queueing thousands of launches
RESIDUAL_LAUNCHES = 1  # launches of one residual (row bands of 64, no partial sums), whatever n is


class PosDefException(Exception):
    """LinearAlgebra.PosDefException(info): the leading minor of order `info` (1-based) is not positive definite."""

    def __init__(self, info: int):
        super().__init__(f"matrix is not positive definite; Factorization failed (leading minor of order {info}).")
        self.info = int(info)


class ZeroPivotException(Exception):
    """LinearAlgebra.ZeroPivotException(info): the unpivoted LDLᵀ met a pivot that is exactly zero or not finite at the
    1-based index `info`, counted from the start of the matrix."""

    def __init__(self, info: int):
        super().__init__(f"ZeroPivotException: factorization encountered one or more zero pivots. Consider switching "
                         f"to a pivoted factorization (first zero or non-finite pivot: {info}).")
        self.info = int(info)


class SingularException(Exception):
    """LinearAlgebra.SingularException(info): the pivoted LU met a pivot that is exactly zero or not finite in column
    `info` (1-based, counted from the start of the matrix), so U is singular."""

    def __init__(self, info: int):
        super().__init__(f"SingularException({info}): matrix is singular to working precision; the pivot of column {info} "
                         f"is zero or not finite.")
        self.info = int(info)


def _check_matrix(M, name: str) -> int:
    """The checks that need no device, in the reference's order: square first, then the element type."""
    if not isinstance(M, torch.Tensor) or M.dim() != 2:
        raise TypeError(f"{name}: M must be a 2-D torch.Tensor on the GPU")
    m, n = M.shape
    if m != n:
        raise LinearOperatorException("shape mismatch")
    if M.dtype.is_complex:
        raise TypeError(f"{name}: real Float64 / Float32 only, got {M.dtype} (complex factorisations are not instantiated)")
    dtype_code(M.dtype)
    if not M.is_cuda:
        raise RuntimeError(f"{name}: M lives on {M.device}: the MI355X path has no CPU fallback")
    return n


def _check_operands(res, v, T):
    if res.dtype is not T or v.dtype is not T:
        raise TypeError(f"mul!: {res.dtype} / {v.dtype} operands next to a {T} factorisation")
    if (res.numel() > 1 and res.stride(0) != 1) or (v.numel() > 1 and v.stride(0) != 1):
        raise ValueError("mul!: res and v must have unit stride")


def _check_block_operands(res, m, T, n, nres=None):
    """The operands of a block apply, as `_apply_closure_to_matrix` hands them over (column-major, any leading
    dimension): V is n x k and res nres x k (nres = n unless given: a rectangular operator). Returns (ldr, ldv, k)."""
    nres = n if nres is None else nres
    if res.dtype is not T or m.dtype is not T:
        raise TypeError(f"mul!: {res.dtype} / {m.dtype} operands next to a {T} factorisation")
    if res.dim() != 2 or m.dim() != 2 or m.shape[0] != n or res.shape[0] != nres or res.shape[1] != m.shape[1]:
        raise LinearOperatorException("shape mismatch")
    k = m.shape[1]
    lds = []
    for X, rows in ((res, nres), (m, n)):
        if rows > 1 and X.stride(0) != 1:
            raise ValueError("mul!: the columns of res and V must have unit stride")
        ldx = X.stride(1) if k > 1 else max(1, rows)
        if ldx < max(1, rows):
            raise ValueError("mul!: res and V must be column-major (leading dimension >= n)")
        lds.append(ldx)
    return lds[0], lds[1], k


def _work(n, device, refine=0):
    """The f64 work matrix of the sweeps, n x GROUP with column stride n: allocated once, at construction. With refine > 0 a
    second one follows it, the iterate x."""
    return torch.empty((2 if refine else 1) * max(1, n) * GROUP, dtype=torch.float64, device=device)


def _check_refine(refine, name: str) -> int:
    """Runs before M is looked at. bool is an int to Python; it is not a step count."""
    if isinstance(refine, bool) or not isinstance(refine, int):
        raise TypeError(f"{name}: refine must be an int, got {type(refine).__name__}")
    if not 0 <= refine <= MAX_REFINE:
        raise ValueError(f"{name}: refine = {refine} outside 0 .. MAX_REFINE = {MAX_REFINE}")
    return refine


def _refined(vec_call):
    """prod and its block form for refine > 0: `vec_call(res, ldr, V, ldv, k, a, b)` is the block-shaped entry point, k = 1
    the vector apply."""
    def prod(res, v, a, b, T, n):
        _check_operands(res, v, T)
        ld = max(1, n)
        vec_call(res, ld, v, ld, 1, a, b)

    def block(res, m, a, b, T, n):
        ldr, ldv, k = _check_block_operands(res, m, T, n)
        vec_call(res, ldr, m, ldv, k, a, b)
    return prod, block


_REFINE_DOC = """

    refine = r (an int, 0 <= r <= MAX_REFINE; 0: the plain solve, launch for launch): every apply computes x₀ = F \\ v, then r
    times x += F \\ (v − M x), and res = α x_r + β res. The residual and every x are Float64 for both element types; the
    one rounding to the element type is in the epilogue. The step count is fixed: no convergence test, nothing is read
    back, so the apply still allocates nothing, never synchronises and can be captured. Refinement converges when the
    plain solve is contractive, roughly ρ·cond·eps(T) < 1 (ρ the growth of the factorisation); when it is not, the iterates
    may not improve and nothing reports it. The exceptions of the factorisation are raised as before."""


def _two_mode(T, nrows, ncols, symm, herm, solve, block, fwd, bwd, device):
    """The operator whose applies take an op_mode: prod! is `solve` / `block` (the matrix form) in mode fwd, tprod! = ctprod!
    in mode bwd."""
    prod = columnwise(lambda res, v, a, b: solve(res, v, a, b, fwd))       # mulFact!(res, F, v, α, β) — src/linalg.jl:3-9
    tprod = columnwise(lambda res, u, a, b: solve(res, u, a, b, bwd))      # mulFact!(res, transpose(F), u, α, β)
    prod._matrix = lambda res, m, a, b: block(res, m, a, b, fwd)
    tprod._matrix = lambda res, m, a, b: block(res, m, a, b, bwd)
    return LinearOperator(T, nrows, ncols, bool(symm), bool(herm), prod, tprod, tprod, S=Storage(T, device))


def _symmetric(name, stem, factor, pivots, exception, M, check, refine):
    """opCholesky (`mxlo_potrf`, the `mxlo_chol_mul*` applies) and opLDL (`mxlo_ldlt`, `mxlo_ldl_mul*`, with the pivots d
    after the block inverses in every call): the checks in the reference's order, the storage, the factorisation, whose
    info != 0 raises `exception`, and the closures."""
    refine = _check_refine(refine, name)
    n = _check_matrix(M, name)
    T = M.dtype
    if check:
        from .utilities import check_hermitian, check_positive_definite
        if not check_hermitian(M):
            raise LinearOperatorException("matrix is not Hermitian")
        if not pivots and not check_positive_definite(M):              # opLDL has no definiteness check
            raise LinearOperatorException("matrix is not positive definite")
    St, tr = _stored_colmajor(M)                       # tr: St is the column-major storage of Mᵀ, i.e. M is row-major
    ldm = max(1, St.stride(1)) if n > 1 else 1
    ctx = get_ctx(M.device)
    W = torch.zeros((n, n), dtype=T, device=M.device).t()            # column-major, ld = n; the lower triangle is L (opLDL: L D)
    ldw = max(1, n)
    nblk = (n + BLOCK - 1) // BLOCK
    dinv = torch.empty(max(1, nblk) * BLOCK * BLOCK, dtype=torch.float64, device=M.device)
    d = torch.empty(n, dtype=torch.float64, device=M.device) if pivots else None
    work = _work(n, M.device, refine)
    info_dev = torch.zeros(1, dtype=torch.int32, device=M.device)
    info = C.c_int32(0)
    code = dtype_code(T)
    piv = (d.data_ptr(),) if pivots else ()
    _lib.call(factor, ctx.handle, code, St.data_ptr(), ldm, 1 if tr else 0, W.data_ptr(), ldw, n, dinv.data_ptr(), *piv,
              info_dev.data_ptr(), C.byref(info))
    if info.value != 0:
        raise exception(info.value)
    pW, pZ = W.data_ptr(), work.data_ptr()
    head = (pW, ldw, n, dinv.data_ptr()) + piv
    mul, mul_block, mul_refine = f"mxlo_{stem}_mul", f"mxlo_{stem}_mul_block", f"mxlo_{stem}_mul_refine"
    if refine:                                          # the snapshot: after the chain, which leaves the strict upper triangle alone
        dg = torch.empty(max(1, n), dtype=T, device=M.device)
        _lib.call("mxlo_sym_snapshot", ctx.handle, code, St.data_ptr(), ldm, 1 if tr else 0, pW, ldw, n, dg.data_ptr())
        pG = dg.data_ptr()

    def prod(res, v, a, b):                             # mulFact!(res, F, v, α, β) — src/linalg.jl:3-9
        _check_operands(res, v, T)
        _lib.call(mul, ctx_of(res).handle, code, res.data_ptr(), *head, pZ, v.data_ptr(), float(a), float(b))

    def block(res, m, a, b):                            # `F \ V`: one chain of launches and one read of L per 8 columns
        ldr, ldv, k = _check_block_operands(res, m, T, n)
        _lib.call(mul_block, ctx_of(res).handle, code, res.data_ptr(), ldr, *head, pZ, m.data_ptr(), ldv, k, float(a), float(b))

    if refine:
        rprod, rblock = _refined(lambda res, ldr, V, ldv, k, a, b: _lib.call(
            mul_refine, ctx_of(res).handle, code, res.data_ptr(), ldr, *head, pG, pZ, V.data_ptr(), ldv, k, refine, float(a), float(b)))
        prod = lambda res, v, a, b: rprod(res, v, a, b, T, n)                   # noqa: E731
        block = lambda res, m, a, b: rblock(res, m, a, b, T, n)                 # noqa: E731
    columnwise(prod)                                    # `F \ V` takes matrices: k == 1 column by column, else the block form
    prod._matrix = block
    op = LinearOperator(T, n, n, True, True, prod, prod, prod, S=Storage(T, M.device))      # isreal(M), hermitian = true
    op._deps = (W,)
    if pivots:
        op._d = d                                       # the pivots; their signs are the inertia of M
    op._factor = (W, dinv) + ((d,) if pivots else ()) + (work,) + ((dg,) if refine else ())   # owned storage (kept alive with the operator)
    op._refine = refine
    return op


def opCholesky(M: torch.Tensor, check: bool = False, refine: int = 0):


    """opCholesky(M; check=false) — src/linalg.jl:44-58: the inverse of a symmetric positive definite matrix through its
    Cholesky factorisation, computed ONCE here, on the device, into storage the operator owns (M is not modified).

    Like `cholesky(M)` = `cholesky(Hermitian(M, :U))`, only the UPPER triangle of M is read; column-major and row-major
    M are read in place, anything else is copied to column-major first. A pivot that is not positive and finite raises
    `PosDefException(info)` with the 1-based order of the failing leading minor. `check=True` runs `check_hermitian`
    and `check_positive_definite` first. prod! = tprod! = ctprod!: res = α (M⁻¹ v) + β res; with β == 0 res is not
    read; res may be v. An apply allocates nothing and never synchronises, so it can be captured (`capture_mul`). Matrix
    operands (n x k, k > 1) go through `mxlo_chol_mul_block`: 8 columns per chain of launches; res may be V.

    With refine > 0 the operator keeps a snapshot of M, taken here: its strict upper triangle in the unused strict upper
    triangle of the factor's storage, its diagonal in n further elements — no second n x n buffer; the work space is 2 n x 8
    doubles. A later change of M is not seen, as before."""
    return _symmetric("opCholesky", "chol", "mxlo_potrf", False, PosDefException, M, check, refine)


opCholesky.__doc__ += _REFINE_DOC


def opLDL(M: torch.Tensor, check: bool = False, refine: int = 0, pivot: bool = False):
    """opLDL(M; check=false) — ext/LinearOperatorsLDLFactorizationsExt.jl:5-18 (docstring: src/linalg.jl:60-73) for a DENSE
    symmetric M: its inverse through M = L D Lᵀ (L unit lower triangular, D diagonal), computed ONCE here, on the device,
    into storage the operator owns (M is not modified). Only the UPPER triangle of M is read (`Symmetric(M, :U)`);
    column-major and row-major M are read in place, anything else is copied to column-major first. `check=True` runs
    `check_hermitian` first; there is no definiteness check.

    pivot=True (a bool, checked before M is looked at): Pᵀ M P = L D Lᵀ by Bunch–Kaufman partial pivoting, LAPACK's `sytrf`
    strategy with α = (1 + √17)/8: D is block diagonal with 1 x 1 and 2 x 2 blocks, |L| stays bounded, and the solve is
    backward stable for ANY symmetric M that is not singular — [[0, 1], [1, 0]] and saddle-point matrices [0 B; Bᵀ A]
    included. The pivot search, the four-way decision and the symmetric interchanges happen on the device inside a chain
    of 3⌈n/64⌉ + 1 launches that depends on n only (`mxlo_sytrf`; panels of 64 or 65 columns); an n x 65
    workspace lives during the construction. `op._perm` (int32, device): M[perm][:, perm] = L D Lᵀ; `op._d` the diagonal of
    D and `op._e` its sub-diagonal (Float64; e[k] ≠ 0 exactly where a 2 x 2 block occupies k, k + 1); `op._factor[0]` holds the
    fully permuted L strictly below its diagonal. `ldl_inertia(op)` counts the inertia of M from d and e.
    `ZeroPivotException(info)`: at the step that starts at the 1-based column info, max(|a_kk|, λ) of a 1 x 1 step, or the
    determinant of a 2 x 2 step, is exactly zero or not finite. An apply is `ldlp_launches(n)` = 2⌈n/64⌉ + 1 launches (gather
    by perm, the sweep with L, one element-wise launch for D⁻¹, the sweep with Lᵀ, the epilogue scattered by perm), with
    every promise below; matrix operands take the block form (`mxlo_ldlp_mul_block`). refine > 0 with pivot=True is a
    ValueError. What follows describes pivot=False, which is unchanged.

    Without pivot=True there is NO pivoting: no symmetric permutation and no 2 x 2 (Bunch–Kaufman) pivots. The factorisation is taken "if it
    exists", in the order the rows come, which keeps it a fixed chain of launches without a host round trip. Negative
    pivots and tiny non-zero pivots are legitimate and are used as they come; a pivot that is exactly zero or not finite
    raises `ZeroPivotException(info)` with its 1-based index. The solve is backward stable when
    ‖ |L||D||Lᵀ| ‖ / ‖M‖ is modest, which holds for symmetric quasi-definite matrices [A Bᵀ; B −C] (A, C positive
    definite) in any symmetric permutation, and for definite ones; for a general indefinite M it need not be.

    prod! = tprod! = ctprod!: res = α (M⁻¹ v) + β res; with β == 0 res is not read; res may be v. An apply allocates
    nothing and never synchronises, so it can be captured (`capture_mul`). `op._d` is a Float64 device tensor with the n
    pivots (the diagonal of D): by Sylvester's law of inertia their signs are the inertia of M.

    refine > 0 is the cure for a general indefinite M that stays inside the fixed chain of launches: one step brings the
    backward error from ρ·eps (ρ the growth of |L||D||Lᵀ|) back to the order of n·eps as long as ρ·cond·eps < 1. The
    operator then keeps a snapshot of M, taken here: its strict upper triangle in the unused strict upper triangle of the
    factor's storage, its diagonal in n further elements — no second n x n buffer; the work space is 2 n x 8 doubles."""
    if not isinstance(pivot, bool):                     # before M is looked at, as _check_refine / _check_pivot
        raise TypeError(f"opLDL: pivot must be a bool, got {type(pivot).__name__}")
    if not pivot:
        return _symmetric("opLDL", "ldl", "mxlo_ldlt", True, ZeroPivotException, M, check, refine)
    if _check_refine(refine, "opLDL"):
        raise ValueError("opLDL: refine > 0 is not provided for pivot=True (DESIGN.md §8)")
    return _ldl_pivoted(M, check)


opLDL.__doc__ += _REFINE_DOC


def ldlp_launches(n: int) -> int:
    """Launches of ONE apply of opLDL(M, pivot=True) of order n: the ⌈n/64⌉ of the sweep with L, one for D⁻¹, the ⌈n/64⌉ of the
    sweep with Lᵀ. It depends on n only, whatever the pivots are."""
    n = int(n)
    return 0 if n <= 0 else 2 * ((n + BLOCK - 1) // BLOCK) + 1


def ldlp_block_launches(n: int, k: int) -> int:
    """Launches of a pivoted apply to a matrix with k columns: the chain of one vector apply per group of GROUP columns."""
    return ((int(k) + GROUP - 1) // GROUP) * ldlp_launches(n)


def _ldl_pivoted(M, check):
    """opLDL(M, pivot=True) once `pivot` and `refine` have been checked: `_symmetric`'s order of checks, the storage, `mxlo_sytrf`,
    the closures over `mxlo_ldlp_mul` / `mxlo_ldlp_mul_block`."""
    n = _check_matrix(M, "opLDL")
    T = M.dtype
    if check:
        from .utilities import check_hermitian
        if not check_hermitian(M):
            raise LinearOperatorException("matrix is not Hermitian")
    St, tr = _stored_colmajor(M)
    ldm = max(1, St.stride(1)) if n > 1 else 1
    ctx = get_ctx(M.device)
    W = torch.zeros((n, n), dtype=T, device=M.device).t()            # column-major, ld = n: L strictly below the diagonal
    ldw = max(1, n)
    nblk = (n + BLOCK - 1) // BLOCK
    dinv = torch.empty(max(1, nblk) * BLOCK * BLOCK, dtype=torch.float64, device=M.device)
    de = torch.zeros((2, max(1, n)), dtype=torch.float64, device=M.device)    # the diagonal and the sub-diagonal of D
    pbuf = torch.empty(2 * n + nblk + 1, dtype=torch.int32, device=M.device)  # the permutation, the interchanges, the panel starts
    panel = torch.empty(max(1, n) * (BLOCK + 1), dtype=T, device=M.device)    # L D of one panel: needed by the factorisation only
    work = _work(n, M.device)
    info_dev = torch.zeros(1, dtype=torch.int32, device=M.device)
    info = C.c_int32(0)
    code = dtype_code(T)
    _lib.call("mxlo_sytrf", ctx.handle, code, St.data_ptr(), ldm, 1 if tr else 0, W.data_ptr(), ldw, n, dinv.data_ptr(),
              de[0].data_ptr(), de[1].data_ptr(), pbuf.data_ptr(), panel.data_ptr(), info_dev.data_ptr(), C.byref(info))
    del panel                                           # after the read-back of info, which is the end of the chain
    if info.value != 0:
        raise ZeroPivotException(info.value)
    head = (W.data_ptr(), ldw, n, dinv.data_ptr(), de[0].data_ptr(), de[1].data_ptr(), pbuf.data_ptr(), work.data_ptr())

    def prod(res, v, a, b):                             # mulFact!(res, F, v, α, β) — src/linalg.jl:3-9
        _check_operands(res, v, T)
        _lib.call("mxlo_ldlp_mul", ctx_of(res).handle, code, res.data_ptr(), *head, v.data_ptr(), float(a), float(b))

    def block(res, m, a, b):                            # `F \ V`: one chain of launches and two reads of L per 8 columns
        ldr, ldv, k = _check_block_operands(res, m, T, n)
        _lib.call("mxlo_ldlp_mul_block", ctx_of(res).handle, code, res.data_ptr(), ldr, *head, m.data_ptr(), ldv, k, float(a), float(b))

    columnwise(prod)
    prod._matrix = block
    op = LinearOperator(T, n, n, True, True, prod, prod, prod, S=Storage(T, M.device))
    op._deps = (W,)
    op._perm = pbuf[:n]
    op._d = de[0, :n]
    op._e = de[1, :n]
    op._factor = (W, dinv, de, pbuf, work)              # owned storage (kept alive with the operator)
    op._refine = 0
    return op


def ldl_inertia(op):
    """(n_pos, n_neg, n_zero) of the matrix an opLDL operator was built from, by Sylvester's law of inertia from the block
    diagonal D: one read-back of `op._d` and, for a pivoted operator, `op._e`. A 2 x 2 block that Bunch–Kaufman chose has a
    negative determinant, one positive and one negative eigenvalue, and counts (1, 1, 0). An unpivoted operator has no
    `_e`: its D is diagonal."""
    d = getattr(op, "_d", None)
    if d is None:
        raise TypeError("ldl_inertia: not an opLDL operator (no pivots `_d`)")
    e = getattr(op, "_e", None)
    d = d.detach().cpu().tolist() if e is None else torch.stack((d, e)).cpu().tolist()
    d, e = (d, [0.0] * len(d)) if e is None else d
    pos = neg = zero = 0
    k, n = 0, len(d)
    while k < n:
        if e[k] != 0.0 and k + 1 < n:
            pos, neg, k = pos + 1, neg + 1, k + 2
            continue
        pos, neg, zero = pos + (d[k] > 0), neg + (d[k] < 0), zero + (d[k] == 0)
        k += 1
    return int(pos), int(neg), int(zero)


def opInverse(M: torch.Tensor, symm: bool = False, herm: bool = False):
    """opInverse(M; symm=false, herm=false) — src/linalg.jl:27-32, for a TRIANGULAR M: each apply is a triangular solve.

    Whether M is lower or upper triangular is decided here, once, on the device (strict upper / strict lower part
    exactly zero — the test dense `\\` makes; a diagonal M counts as lower). A square M that is neither raises: general
    dense opInverse needs a pivoted LU, which is `opLU(M)`, not this constructor. M is ALIASED (column-major or row-major
    storage; any other striding is copied once): a later in-place change of its values is seen by the next apply — the
    inverses of its 64 x 64 diagonal blocks are cached under `state_version(M)` and rebuilt (one launch) when it
    changes. The triangle kind stays what it was at construction. prod! solves with M, tprod! / ctprod! with Mᵀ.
    A zero on the diagonal is NOT detected: the result then holds Inf / NaN and no exception is raised, as with the
    reference's triangular `\\` on a device array. res may be v; with β == 0 res is not read."""
    n = _check_matrix(M, "opInverse")
    T = M.dtype
    St, tr = _stored_colmajor(M)
    ld = max(1, St.stride(1)) if n > 1 else 1
    ctx = get_ctx(M.device)
    code = dtype_code(T)
    kind_dev = torch.zeros(1, dtype=torch.int32, device=M.device)
    _lib.call("mxlo_tri_kind", ctx.handle, code, St.data_ptr(), ld, n, kind_dev.data_ptr())
    bits = int(kind_dev.item())                         # the one read of the device word
    if bits == 3:
        raise LinearOperatorException("opInverse: M is neither lower nor upper triangular; a general dense inverse needs a "
                                      "pivoted LU: use opLU(M); opInverse is triangular-only")
    st_upper = bits == 1                                # of the stored matrix; bits == 0 (diagonal) counts as lower
    nblk = (n + BLOCK - 1) // BLOCK
    dinv = torch.empty(max(1, nblk) * BLOCK * BLOCK, dtype=torch.float64, device=M.device)
    work = _work(n, M.device)
    pT, pD, pZ = St.data_ptr(), dinv.data_ptr(), work.data_ptr()
    cache = {"version": None}

    def prepare(h):
        ver = state_version(St)
        if ver != cache["version"]:                     # M changed in place: its diagonal blocks' inverses are stale
            _lib.call("mxlo_tri_prepare", h, code, pT, ld, n, 1 if st_upper else 0, pD)
            cache["version"] = ver

    def solve(res, v, a, b, mode):
        _check_operands(res, v, T)
        h = ctx_of(res).handle
        prepare(h)
        _lib.call("mxlo_trisolve_mul", h, code, res.data_ptr(), pT, ld, n, 1 if st_upper else 0, mode, pD, pZ, v.data_ptr(),
                  float(a), float(b))

    def block(res, m, a, b, mode):
        ldr, ldv, k = _check_block_operands(res, m, T, n)
        h = ctx_of(res).handle
        prepare(h)
        _lib.call("mxlo_trisolve_mul_block", h, code, res.data_ptr(), ldr, pT, ld, n, 1 if st_upper else 0, mode, pD, pZ,
                  m.data_ptr(), ldv, k, float(a), float(b))

    fwd, bwd = (_lib.OP_T, _lib.OP_N) if tr else (_lib.OP_N, _lib.OP_T)
    op = _two_mode(T, n, n, symm, herm, solve, block, fwd, bwd, M.device)
    op._deps = (M,)
    op._triangle = "lower" if (bits == 0 or st_upper == tr) else "upper"   # of M itself
    op._factor = (St, dinv, work)
    return op


def opLU(M: torch.Tensor, symm: bool = False, herm: bool = False, refine: int = 0):
    """opLU(M; symm=false, herm=false): the inverse of a GENERAL square dense M, what `opInverse(M)` = `M \\ v` of
    src/linalg.jl:27-32 is for a full matrix — through P M = L U with partial pivoting, computed ONCE here, on the device,
    into storage the operator owns (M is not modified; a later change of M is not seen).

    The pivot of column j is the first row i >= j with the largest |a_ij| over the whole remaining column, found on the
    device inside the chain of launches: no host round trip, and |L_ij| <= 1. Column-major M is read as it lies; a
    row-major M is the column-major storage of Mᵀ, which is factored as it lies with prod! and tprod! exchanged; any other
    striding is copied once. A pivot that is exactly zero or not finite raises `SingularException(info)` with its
    1-based column HERE, at construction; the reference factors inside `\\` and so raises it at the first apply.
    symm / herm are taken as given, as `opInverse` takes them.

    prod!: res = α (M⁻¹ v) + β res; tprod! = ctprod!: with Mᵀ. With β == 0 res is not read; res may be v. An apply is
    2⌈n/64⌉ − 1 launches and nothing else, so it can be captured (`capture_mul`). `op._perm` is the int32 device
    permutation, M[op._perm[i], :] = (L U)[i, :] for the stored matrix; `op._factor[0]` holds L (unit, strictly below the
    diagonal) and U.

    With refine > 0 the operator owns a SECOND n x n matrix, which doubles its memory: the factor's storage holds both L and
    U, so the snapshot of the stored matrix the residual reads has no free triangle to live in. It is kept with its rows in
    pivot order (P M), so that a step's residual comes out in the order the sweeps work in. The work space is 2 n x 8
    doubles. prod!, tprod! and ctprod! all refine, each with its own op(M)."""
    refine = _check_refine(refine, "opLU")
    n = _check_matrix(M, "opLU")
    T = M.dtype
    St, tr = _stored_colmajor(M)                       # tr: St is the column-major storage of Mᵀ
    ldm = max(1, St.stride(1)) if n > 1 else 1
    ctx = get_ctx(M.device)
    W = torch.empty((n, n), dtype=T, device=M.device).t()            # column-major, ld = n: L below the diagonal, U on and above
    ldw = max(1, n)
    nblk = (n + BLOCK - 1) // BLOCK
    dinv_l = torch.empty(max(1, nblk) * BLOCK * BLOCK, dtype=torch.float64, device=M.device)
    dinv_u = torch.empty_like(dinv_l)
    pbuf = torch.empty(max(1, 2 * n), dtype=torch.int32, device=M.device)     # the permutation, then LAPACK's ipiv (0-based)
    work = _work(n, M.device, refine)
    info_dev = torch.zeros(1, dtype=torch.int32, device=M.device)
    info = C.c_int32(0)
    code = dtype_code(T)
    _lib.call("mxlo_getrf", ctx.handle, code, St.data_ptr(), ldm, W.data_ptr(), ldw, n, dinv_l.data_ptr(), dinv_u.data_ptr(),
              pbuf.data_ptr(), info_dev.data_ptr(), C.byref(info))
    if info.value != 0:
        raise SingularException(info.value)
    pW, pL, pU, pP, pZ = W.data_ptr(), dinv_l.data_ptr(), dinv_u.data_ptr(), pbuf.data_ptr(), work.data_ptr()
    if refine:                                          # the snapshot: the stored matrix, rows in pivot order
        A2 = torch.empty((n, n), dtype=T, device=M.device).t()
        _lib.call("mxlo_lu_snapshot", ctx.handle, code, St.data_ptr(), ldm, pP, A2.data_ptr(), ldw, n)
        pA = A2.data_ptr()

    def solve(res, v, a, b, mode):                      # mulFact!(res, lu(M), v, α, β) — src/linalg.jl:3-9
        _check_operands(res, v, T)
        _lib.call("mxlo_lu_mul", ctx_of(res).handle, code, res.data_ptr(), pW, ldw, n, pL, pU, pP, pZ, v.data_ptr(), mode,
                  float(a), float(b))

    def block(res, m, a, b, mode):
        ldr, ldv, k = _check_block_operands(res, m, T, n)
        _lib.call("mxlo_lu_mul_block", ctx_of(res).handle, code, res.data_ptr(), ldr, pW, ldw, n, pL, pU, pP, pZ, m.data_ptr(), ldv,
                  k, mode, float(a), float(b))

    if refine:
        def refined(mode):
            return _refined(lambda res, ldr, V, ldv, k, a, b: _lib.call(
                "mxlo_lu_mul_refine", ctx_of(res).handle, code, res.data_ptr(), ldr, pW, ldw, n, pL, pU, pP, pA, ldw, pZ, V.data_ptr(),
                ldv, k, refine, mode, float(a), float(b)))
        rs = {_lib.OP_N: refined(_lib.OP_N), _lib.OP_T: refined(_lib.OP_T)}
        solve = lambda res, v, a, b, mode: rs[mode][0](res, v, a, b, T, n)      # noqa: E731
        block = lambda res, m, a, b, mode: rs[mode][1](res, m, a, b, T, n)      # noqa: E731
    fwd, bwd = (_lib.OP_T, _lib.OP_N) if tr else (_lib.OP_N, _lib.OP_T)
    op = _two_mode(T, n, n, symm, herm, solve, block, fwd, bwd, M.device)
    op._deps = (W,)
    op._perm = pbuf[:n]
    op._factor = (W, dinv_l, dinv_u, pbuf, work) + ((A2,) if refine else ())    # owned storage (kept alive with the operator)
    op._refine = refine
    return op


opLU.__doc__ += _REFINE_DOC


QR_SLOTS = 512        # most workgroups of a pass over the rows (QG of csrc/linalg.hip): partial slots per column
QRP_SLOTS = 64        # most row groups of a step of the pivoted factorisation (QPG of csrc/linalg.hip)


def geqrf_scratch(nf: int) -> int:
    """Doubles of the scratch of `mxlo_geqrf` (and of `mxlo_cod_factor`, with nf := rank): geqrf_scratch() of csrc/linalg.hip."""
    return 2 * (QR_SLOTS * BLOCK + BLOCK) + (QR_SLOTS + 2 * ((nf + BLOCK - 1) // BLOCK)) * BLOCK * BLOCK


def geqp3_scratch(mf: int, nf: int) -> int:
    """Doubles of the scratch of `mxlo_geqp3`: geqp3_scratch() of csrc/linalg.hip."""
    return 2 * QRP_SLOTS * nf + QRP_SLOTS + 2 * nf + 2 * mf + 2 + QRP_SLOTS * BLOCK * BLOCK


def qr_block_work(mf: int, nf: int) -> int:
    """Doubles of the work space of the rectangular applies — the block apply's: z (mf x GROUP), two sets of partial slots per
    column, the sweep's nf x GROUP; the vector apply uses a prefix: qr_block_work() of csrc/linalg.hip."""
    return GROUP * (mf + nf + 2 * QR_SLOTS * BLOCK)


def _rect_storage(T, rows, cols, device, zero_dinv=False, work=True, info_words=1):
    """What a factorisation of the rectangular family fills and its operator owns: W (rows x cols column-major, ld = rows), the
    T factors (zero where no block column writes them), the block inverses of R, the applies' work space, the info words."""
    nblk = (cols + BLOCK - 1) // BLOCK
    W = torch.empty((cols, rows), dtype=T, device=device).t()
    tfac = torch.zeros(nblk * BLOCK * BLOCK, dtype=torch.float64, device=device)
    dinv = (torch.zeros if zero_dinv else torch.empty)(nblk * BLOCK * BLOCK, dtype=torch.float64, device=device)
    wk = torch.empty(qr_block_work(rows, cols), dtype=torch.float64, device=device) if work else None
    info_dev = torch.zeros(info_words, dtype=torch.int32, device=device)
    return W, tfac, dinv, wk, info_dev


def _rect_operator(T, m, k, tall, mf, nf, vec_name, block_name, W, mid, work):
    """The k x m operator of a factored tall orientation F (mf x nf; W with ld = mf): `vec_name` and `block_name` are its
    entry points, `mid` the arguments between `ldw, mf, nf` and the work pointer."""
    code = dtype_code(T)
    head = (W.data_ptr(), mf, mf, nf) + tuple(mid) + (work.data_ptr(),)

    def solve(res, v, a, b, mode):                      # mulFact!(res, qr(F), v, α, β) — src/linalg.jl:3-9
        _check_operands(res, v, T)
        _lib.call(vec_name, ctx_of(res).handle, code, res.data_ptr(), *head, v.data_ptr(), mode, float(a), float(b))

    def block(res, V, a, b, mode):
        nv, nres = (mf, nf) if mode == _lib.OP_N else (nf, mf)
        ldr, ldv, cols = _check_block_operands(res, V, T, nv, nres)
        _lib.call(block_name, ctx_of(res).handle, code, res.data_ptr(), ldr, *head, V.data_ptr(), ldv, cols, mode, float(a), float(b))

    fwd, bwd = (_lib.OP_N, _lib.OP_T) if tall else (_lib.OP_T, _lib.OP_N)
    op = _two_mode(T, k, m, False, False, solve, block, fwd, bwd, W.device)
    op._deps = (W,)
    op._tall = tall
    return op


def qr_launches(nf: int) -> int:
    """Launches of ONE opQR apply, in either mode, for a factor with nf columns: ⌈nf/64⌉ + 1 reflector launches and the
    ⌈nf/64⌉ of the sweep with R. It does not depend on the number of rows."""
    return 2 * ((int(nf) + BLOCK - 1) // BLOCK) + 1


def qr_block_launches(nf: int, k: int) -> int:
    """Launches of an opQR apply to a matrix with k columns: the chain of one vector apply per group of GROUP columns."""
    return ((int(k) + GROUP - 1) // GROUP) * qr_launches(nf)


def _check_rect(A, name: str):
    """opQR's checks that need no device, in the order the docstring states. Rectangular is not a shape mismatch."""
    if not isinstance(A, torch.Tensor) or A.dim() != 2:
        raise TypeError(f"{name}: A must be a 2-D torch.Tensor on the GPU")
    m, k = A.shape
    if m == 0 or k == 0:
        raise LinearOperatorException(f"{name}: a {m} x {k} matrix has no QR solve")
    if A.dtype not in (torch.float64, torch.float32):
        raise TypeError(f"{name}: real Float64 / Float32 only, got {A.dtype} (complex and half factorisations are not instantiated)")
    if not A.is_cuda:
        raise RuntimeError(f"{name}: A lives on {A.device}: the MI355X path has no CPU fallback")
    return m, k


def qrp_launches(rank: int) -> int:
    """Launches of ONE apply of opQR(A, pivot=True) whose numerical rank is `rank`, in either mode: those of the unpivoted
    apply of a factor with `rank` columns. The entries of a rank-deficient solution that are no pivots are written by the
    last reflector launch, so the launch the contract allows for them is not spent."""
    return qr_launches(rank)


def qrp_block_launches(rank: int, k: int) -> int:
    """Launches of a pivoted apply to a matrix with k columns: the chain of one vector apply per group of GROUP columns."""
    return ((int(k) + GROUP - 1) // GROUP) * qrp_launches(rank)


def _check_pivot(pivot, rtol, name: str):
    """Runs before A is looked at. Returns rtol as a float, or None for the default."""
    if not isinstance(pivot, bool):
        raise TypeError(f"{name}: pivot must be a bool, got {type(pivot).__name__}")
    if rtol is None:
        return None
    if isinstance(rtol, bool) or not isinstance(rtol, numbers.Real):
        raise TypeError(f"{name}: rtol must be None or a real number, got {type(rtol).__name__}")
    if not pivot:
        raise ValueError(f"{name}: rtol is the rank tolerance of the pivoted factorisation; it needs pivot=True")
    if not 0 <= rtol < 1:                               # false for NaN as well
        raise ValueError(f"{name}: rtol = {rtol} outside 0 <= rtol < 1")
    return float(rtol)


def _qr_pivoted(A, m, k, rtol):
    """opQR(A, pivot=True) once the checks have passed; the storage is opQR's, with the permutation"""
    T = A.dtype
    tall = m >= k
    mf, nf = (m, k) if tall else (k, m)
    if rtol is None:
        rtol = max(mf, nf) * float(torch.finfo(T).eps)
    St, tr = _stored_colmajor(A)
    m_trans = tall == tr
    ldm = St.stride(1) if St.shape[1] > 1 else max(1, St.shape[0])
    ctx = get_ctx(A.device)
    W, tfac, dinv, work, info_dev = _rect_storage(T, mf, nf, A.device, zero_dinv=True, info_words=2)
    perm = torch.empty(nf, dtype=torch.int32, device=A.device)
    nscratch = geqp3_scratch(mf, nf)
    scratch = torch.empty(nscratch, dtype=torch.float64, device=A.device)                   # needed by the factorisation only
    info, rank = C.c_int32(0), C.c_int32(0)
    _lib.call("mxlo_geqp3", ctx.handle, dtype_code(T), St.data_ptr(), ldm, 1 if m_trans else 0, W.data_ptr(), mf, mf, nf,
              tfac.data_ptr(), dinv.data_ptr(), perm.data_ptr(), rtol, scratch.data_ptr(), nscratch, info_dev.data_ptr(),
              C.byref(info), C.byref(rank))
    if info.value != 0:
        raise SingularException(info.value)
    r = int(rank.value)
    # the T factors and the block inverses are made after the read-back, out of the scratch, on the stream the scratch was
    # allocated on: the allocator hands its memory only to work that this stream runs later
    del scratch
    op = _rect_operator(T, m, k, tall, mf, nf, "mxlo_qrp_mul", "mxlo_qrp_mul_block", W,
                        (tfac.data_ptr(), dinv.data_ptr(), perm.data_ptr(), r), work)
    op._rank = r
    op._perm = perm
    op._rtol = rtol
    op._factor = (W, tfac, dinv, work, perm)            # owned storage (kept alive with the operator)
    return op


def opQR(A: torch.Tensor, pivot: bool = False, rtol=None):
    """opQR(A): the pseudo-inverse A⁺ of a full-rank dense m x k matrix, a k x m operator — what `opInverse(M)` = `M \\ v` of
    src/linalg.jl:27-32 is for a rectangular M: Julia's QR solve. prod!: res = α (A⁺ v) + β res, the least-squares solution
    of A x ≈ v for m >= k and the minimum-norm solution of A x = v for m < k; tprod! = ctprod!: res = α ((A⁺)ᵀ u) + β res, the
    same pair of problems for Aᵀ. With β == 0 res is not read. Never the normal equations: the condition number is not squared.

    ONE factorisation, computed here, on the device, of the TALL orientation F (F = A if m >= k, else Aᵀ; mf x nf): F = Q R by
    unpivoted Householder reflections in block columns of 64 with compact-WY factors (`mxlo_geqrf`), into storage the
    operator owns. A is not modified and a later change of A is not seen. A row-major wide A is the column-major tall Aᵀ
    and is read as it lies, as a column-major tall A is; a column-major wide A (or row-major tall A) is transposed once while
    it is copied; any other striding is copied first. `op._tall`: was A itself factored? `op._factor` = (W, T, dinv, work):
    W (mf x nf, column-major) holds R on and above its diagonal and the reflector vectors below it, LAPACK's layout.

    A column of F whose norm from the diagonal down is exactly zero or not finite raises `SingularException(info)` with
    its 1-based index in F, here, at construction; a zero sub-column below a non-zero diagonal entry is legitimate (τ = 0).
    The norms are taken without rescaling: data whose squares overflow or underflow Float64 is outside what this handles.

    An apply is `qr_launches(nf)` = 2⌈nf/64⌉ + 1 launches, whatever mf is, and nothing else: it allocates nothing, never
    synchronises, can be captured (`capture_mul`) and is bit-reproducible (every sum in a fixed order in Float64). res may be
    v when m == k. Matrix operands (`A \\ V`, `to_dense`) go through the block form (`mxlo_qr_mul_block`): the chain of ONE vector
    apply per GROUP = 8 columns, `qr_block_launches(nf, k)` launches, every element of a reflector panel loaded once per chunk
    of rows for the whole group, each column bit-identical to its vector apply; res may be V (the same matrix) when m == k.
    The work space, allocated once here, is 8 (mf + nf + 2·512·64) Float64; the vector apply uses its first
    mf + 2·512·64. Without pivoting a rank-deficient A that escapes the exact test above gives a meaningless answer.

    pivot=True: F P = Q R with column pivoting (`mxlo_geqp3`), what Julia's `\\` does for a rectangular matrix. At every step
    the pivot is the remaining column of largest 2-norm from the diagonal row down, the first one on a tie; the norms are
    recomputed at every step, never downdated. One column per step, three launches per step, 3 nf + 3 in all, nothing read
    back in between: BLAS-2 work, about 2·sizeof(T)·Σ_c (mf − c)(nf − c) bytes, paid once here. The numerical rank r is the
    length of the leading run of j with |R_jj| > rtol·|R_11|; rtol defaults to max(mf, nf)·eps(T) and must satisfy
    0 <= rtol < 1 (rtol without pivot=True is a ValueError). The rank is decided on the device and read back together with
    the info word, the one synchronisation of the construction. `op._rank` = r, `op._perm` (int32, device, nf entries):
    F[:, op._perm[j]] is column j of Q R, `op._rtol`; `op._factor` = (W, T, dinv, work, perm). A rank-deficient A, zero columns
    included, raises nothing; `SingularException(info)` only when a remaining column norm at step info is not finite (a NaN
    counts as the largest), or info = 1 for A == 0.
    The solves are the BASIC solution of rank r: prod! of a tall A gives x[perm[0:r]] = R11⁻¹ (Qᵀv)[0:r] with the other
    nf − r entries exactly zero before the α, β epilogue; the transposed mode gives y = Q[:, 0:r] R11⁻ᵀ u[perm[0:r]]. For r = nf
    these are the unique least-squares / minimum-norm solutions, as without pivoting. For r < nf they are A least-squares
    solution and, when the system is consistent, A solution — NOT the minimum-norm ones that Julia's complete orthogonal
    decomposition returns (the further `tzrzf` step is not provided). `opPinv(A)` returns the minimum-norm ones. An apply runs the unpivoted apply's kernels on the
    leading r columns, `qrp_launches(r)` = `qr_launches(r)` launches (`qrp_block_launches(r, k)` for a matrix operand), with
    every promise of the paragraph above.

    NOT provided: `refine`, minimum-norm solutions of rank-deficient problems, complex element types, Julia glue."""
    rtol = _check_pivot(pivot, rtol, "opQR")
    m, k = _check_rect(A, "opQR")
    if pivot:
        return _qr_pivoted(A, m, k, rtol)
    T = A.dtype
    tall = m >= k
    mf, nf = (m, k) if tall else (k, m)
    St, tr = _stored_colmajor(A)                        # tr: St is the column-major storage of Aᵀ
    m_trans = tall == tr                                # St holds Fᵀ: transpose while copying
    ldm = St.stride(1) if St.shape[1] > 1 else max(1, St.shape[0])
    ctx = get_ctx(A.device)
    W, tfac, dinv, work, info_dev = _rect_storage(T, mf, nf, A.device)
    nscratch = geqrf_scratch(nf)
    scratch = torch.empty(nscratch, dtype=torch.float64, device=A.device)                   # needed by the factorisation only
    info = C.c_int32(0)
    _lib.call("mxlo_geqrf", ctx.handle, dtype_code(T), St.data_ptr(), ldm, 1 if m_trans else 0, W.data_ptr(), mf, mf, nf,
              tfac.data_ptr(), dinv.data_ptr(), scratch.data_ptr(), nscratch, info_dev.data_ptr(), C.byref(info))
    del scratch
    if info.value != 0:
        raise SingularException(info.value)
    op = _rect_operator(T, m, k, tall, mf, nf, "mxlo_qr_mul", "mxlo_qr_mul_block", W, (tfac.data_ptr(), dinv.data_ptr()), work)
    op._factor = (W, tfac, dinv, work)                  # owned storage (kept alive with the operator)
    return op


def pinv_launches(rank: int, nf: int) -> int:
    """Launches of ONE opPinv apply, in either mode, for a factor with nf columns of numerical rank `rank`. Full rank: the
    pivoted apply's. rank < nf: two reflector chains of ⌈rank/64⌉ + 1 launches joined by the ⌈rank/64⌉ of the sweep with R₂.
    It does not depend on the number of rows."""
    if int(rank) == int(nf):
        return qrp_launches(rank)
    return 3 * ((int(rank) + BLOCK - 1) // BLOCK) + 2


def pinv_block_launches(rank: int, nf: int, k: int) -> int:
    """Launches of an opPinv apply to a matrix with k columns: the chain of one vector apply per group of GROUP columns."""
    return ((int(k) + GROUP - 1) // GROUP) * pinv_launches(rank, nf)


def opPinv(A: torch.Tensor, rtol=None):
    """opPinv(A): the Moore-Penrose pseudo-inverse A⁺ of a dense m x k matrix of ANY rank, a k x m operator — what Julia's
    `A \\ v` returns for a rectangular A: the MINIMUM-NORM least-squares solution, through a complete orthogonal
    decomposition computed on the device. prod!: res = α (A⁺ v) + β res; tprod! = ctprod!: res = α ((A⁺)ᵀ u) + β res, the same
    for Aᵀ, whether or not u is consistent. With β == 0 res is not read.

    Construction: opQR(A, pivot=True, rtol=rtol)'s factorisation F P = Q₁ R of the tall orientation F (mf x nf) with its rank
    decision r (rtol: None for max(mf, nf)·eps(T), else a real with 0 <= rtol < 1; checked before A is looked at, then
    opQR's refusals in their order). r == nf: the operator IS the pivoted one — the same kernels, launches and bits, and
    `op._factor` = (W, T, dinv, work, perm). r < nf: S = [R₁₁ R₁₂]ᵀ (nf x r, full column rank) is taken out of the leading r
    rows of W and factored S = Q₂ R₂ by the unpivoted block-Householder chain (`mxlo_cod_factor`), so that
    F⁺ = P Q₂ R₂⁻ᵀ [I_r 0] Q₁ᵀ; `op._factor` = (W, T, dinv, work, perm, W2, T2, dinv2), W2 nf x r column-major: one more nf x r
    factor and two ⌈r/64⌉·64² Float64 tables. `op._tall`, `op._rank`, `op._perm`, `op._rtol` as opQR(pivot=True)'s, and its
    exceptions: `SingularException` for A == 0 or a column norm that is not finite; a rank-deficient A raises nothing.

    An apply with r < nf is two reflector chains joined by one sweep with R₂ — Q₁ᵀ, R₂⁻ᵀ, Q₂ with the permutation scattered
    by the last launch's epilogue; transposed: Q₂ᵀ with the permutation gathered by the first launch, R₂⁻¹, Q₁ —
    `pinv_launches(r, nf)` = 3⌈r/64⌉ + 2 launches whatever mf is (`pinv_block_launches(r, nf, k)` for a matrix operand, GROUP
    = 8 columns per chain, each column bit-identical to its vector apply), and nothing else: no allocation, no
    synchronisation, capturable, bit-reproducible (every sum in a fixed order in Float64). res may be v when m == k. The work
    space is opQR's. It streams (mf + nf)·r elements twice where the basic solution streams mf·r twice.

    NOT provided: the structured `tzrzf` form of the second stage (reflectors of length 1 + nf − r), `refine`,
    complex element types, Julia glue, sharding."""
    rtol = _check_pivot(True, rtol, "opPinv")
    m, k = _check_rect(A, "opPinv")
    op = _qr_pivoted(A, m, k, rtol)
    T = A.dtype
    tall, r = op._tall, op._rank
    mf, nf = (m, k) if tall else (k, m)
    if r == nf:
        return op
    W, tfac, dinv, work, perm = op._factor
    ctx = get_ctx(A.device)
    W2, tfac2, dinv2, _, info_dev = _rect_storage(T, nf, r, A.device, work=False)           # column-major nf x r, ld = nf
    nscratch = geqrf_scratch(r)
    scratch = torch.empty(nscratch, dtype=torch.float64, device=A.device)                   # needed by the factorisation only
    info = C.c_int32(0)
    _lib.call("mxlo_cod_factor", ctx.handle, dtype_code(T), W.data_ptr(), mf, nf, r, W2.data_ptr(), tfac2.data_ptr(), dinv2.data_ptr(),
              scratch.data_ptr(), nscratch, info_dev.data_ptr(), C.byref(info))
    del scratch
    if info.value != 0:
        raise SingularException(info.value)
    pinv = _rect_operator(T, m, k, tall, mf, nf, "mxlo_pinv_mul", "mxlo_pinv_mul_block", W,
                          (tfac.data_ptr(), perm.data_ptr(), r, W2.data_ptr(), tfac2.data_ptr(), dinv2.data_ptr()), work)
    pinv._rank = r
    pinv._perm = perm
    pinv._rtol = op._rtol
    pinv._factor = (W, tfac, dinv, work, perm, W2, tfac2, dinv2)        # owned storage (kept alive with the operator)
    return pinv
