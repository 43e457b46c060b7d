"""`estimate_opnorm(B) -> (value, converged)` — declared at src/utilities.jl:319, implemented by the reference's
ext/LinearOperatorsOpNormExt.jl with ARPACK (`eigs` for Hermitian operators, `svds` otherwise, dense `eigen` / `svd` for
n <= 5, `ncv` doubling over `max_attempts` tries, `(NaN, false)` when nothing converged).

Here the Krylov process runs on the device: a restarted Lanczos iteration with full re-orthogonalisation whose basis is
ONE device allocation. Every step is the operator's own `mul!` writing `B v_j` straight into basis column j + 1, followed
by `mxlo_krylov_orth` (Gram–Schmidt twice against columns 0..j, csrc/krylov.hip). Nothing comes back to the host inside a
cycle of `ncv` steps: the coefficients of every step collect in a device buffer that is copied ONCE per cycle, and the
host then solves the small tridiagonal eigenproblem (`lanczos_ritz`, plain numpy). An unconverged cycle restarts
explicitly with the Ritz vector (`mxlo_krylov_combine` into column 0). Real Float64 / Float32 operators only."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .device import ctx_of, dtype_code, ptr
from .operators import adjoint, ishermitian, mul, storage_type, to_dense
from .utilities import _as_operator, _float_op

__all__ = ["estimate_opnorm", "lanczos_ritz"]

_last_cycle_counters = None      # mxlo_debug_counters delta of the most recent Lanczos cycle (read by the contract test)


def lanczos_ritz(alpha, beta, n: int = 1, eps: float = float(np.finfo(np.float64).eps)):
    """The host half of a Lanczos cycle, on numpy arrays alone. `alpha[j]`, `beta[j]` (j < m) are the diagonal entry and the
    norm of the next, not yet normalised, Lanczos vector of step j. The recurrence is truncated at the first breakdown
    `beta[j] <= n * eps * max(|alpha[..j]|, |beta[..j-1]|)` (an invariant subspace: the Ritz values are exact). Returns
    `(theta, y, residual, breakdown_index)`: the eigenvalue of largest magnitude of the tridiagonal matrix (ARPACK's
    `which = :LM`), its unit eigenvector, `beta_last * |y_last|` — for which `|theta - lambda| <= residual` holds with some
    eigenvalue lambda of the operator — and the index of the breakdown or None. Non-finite input gives theta = NaN."""
    alpha = np.asarray(alpha, dtype=np.float64).ravel()
    beta = np.asarray(beta, dtype=np.float64).ravel()
    m = min(alpha.size, beta.size)
    if m == 0:
        raise ValueError("lanczos_ritz needs at least one step")
    breakdown, scale = None, 0.0
    for j in range(m):
        if not (math.isfinite(alpha[j]) and math.isfinite(beta[j])):
            return math.nan, np.full(j + 1, math.nan), math.nan, None
        scale = max(scale, abs(alpha[j]))
        if beta[j] <= n * eps * scale:
            breakdown, m = j, j + 1
            break
        scale = max(scale, abs(beta[j]))
    T = np.diag(alpha[:m])
    if m > 1:
        T += np.diag(beta[:m - 1], 1) + np.diag(beta[:m - 1], -1)
    lam, Y = np.linalg.eigh(T)
    i = int(np.argmax(np.abs(lam)))
    y = Y[:, i]
    return float(lam[i]), y, float(beta[m - 1] * abs(y[-1])), breakdown


def _counters():
    a = (C.c_int64 * 12)()
    _lib.call("mxlo_debug_counters", a)
    return list(a)


class _Lanczos:
    """One attempt's device state: the basis (ncv + 1 columns, leading dimension padded to 16 bytes), the per-step
    coefficient rows and the restart coefficients."""

    def __init__(self, step, n, ncv, T, dev):
        self.step, self.n, self.ncv = step, n, ncv
        per16 = 16 // torch.empty(0, dtype=T).element_size()
        self.ldv = -(-n // per16) * per16
        self.V = torch.empty((ncv + 1) * self.ldv, dtype=T, device=dev)
        self.row = ncv + 2
        self.coef = torch.zeros(ncv * self.row, dtype=torch.float64, device=dev)
        self.y = torch.zeros(ncv + 1, dtype=torch.float64, device=dev)     # [0..ncv): restart coefficients, [ncv]: norm slot
        self.host = np.zeros(ncv * self.row, dtype=np.float64)
        self.code = dtype_code(T)
        self.ctx = ctx_of(self.V)

    def col(self, j):
        return self.V[j * self.ldv: j * self.ldv + self.n]

    def combine(self, k, out_col):
        """column `out_col` <- normalised V[:, 0..k) y"""
        self.ctx.bind_stream()
        _lib.call("mxlo_krylov_combine", self.ctx.handle, self.code, ptr(self.V), self.ldv, self.n, k, ptr(self.y),
                  ptr(self.col(out_col)), self.y.data_ptr() + 8 * self.ncv)

    def start(self, v0):
        self.col(0).copy_(v0)
        self.y[0] = 1.0
        self.combine(1, 0)                                               # normalises column 0 in place, no host round trip

    def cycle(self, m):
        """m Lanczos steps from column 0; (alpha, beta) of the steps, after ONE device-to-host copy."""
        global _last_cycle_counters
        before = _counters()
        ctx, V0, es = self.ctx, self.V.data_ptr(), self.V.element_size()
        for j in range(m):
            w = self.col(j + 1)
            self.step(w, self.col(j))                                    # B v_j (or the Gram operator), written in place
            ctx.bind_stream()
            _lib.call("mxlo_krylov_orth", ctx.handle, self.code, V0, self.ldv, self.n, j + 1, V0 + (j + 1) * self.ldv * es,
                      self.coef.data_ptr() + 8 * j * self.row, _lib.KRYLOV_DGKS)
        _lib.call("mxlo_memcpy_d2h", ctx.handle, self.host.ctypes.data, ptr(self.coef), 8 * m * self.row)
        after = _counters()
        _last_cycle_counters = [b - a for a, b in zip(before, after)]
        rows = self.host[:m * self.row].reshape(m, self.row)
        idx = np.arange(m)
        return rows[idx, idx].copy(), rows[idx, idx + 1].copy()

    def restart(self, y):
        k = len(y)
        self.host[:k] = y
        _lib.call("mxlo_memcpy_h2d", self.ctx.handle, ptr(self.y), self.host.ctypes.data, 8 * k)
        self.combine(k, 0)


def _dense_norm(B, hermitian):
    M = to_dense(B).cpu().numpy().astype(np.float64)
    if hermitian:
        return float(np.max(np.abs(np.linalg.eigvalsh(M)))), True        # ext/LinearOperatorsOpNormExt.jl:42-47
    return float(np.max(np.linalg.svd(M, compute_uv=False))), True       # :91-96


def estimate_opnorm(B, *, tol=None, ncv=None, maxiter: int = 300, max_attempts: int = 3, tiny_dense_threshold: int = 5,
                    generator=None):
    """`estimate_opnorm(B; max_attempts = 3, tiny_dense_threshold = 5) -> (value, converged)`: the operator 2-norm of any
    real operator of the package. Hermitian B: restarted Lanczos on B (start `ncv = min(20, n)`), the answer is
    `|theta|` of the Ritz value of largest magnitude. Otherwise the same iteration on the Gram operator of the smaller
    side (`B'B` if ncol <= nrow, else `B B'`; start `ncv = min(10, min(m, n))`), the answer is `sqrt(max(theta, 0))`.
    Converged when the Ritz residual is at most `tol * |theta|` (default `tol = sqrt(eps(T))`) or the recurrence broke down
    (invariant subspace). At most `maxiter` operator applies per attempt, then `ncv` doubles (clipped to the dimension) for
    at most `max_attempts` attempts; `(nan, False)` when nothing converged — no exception."""
    B = _as_operator(B)
    T = _float_op(B)
    if T.is_complex:
        raise TypeError("estimate_opnorm: complex operators are not supported yet (real Float64 / Float32 only)")
    nrow, ncol = B.size()
    herm = bool(ishermitian(B)) and nrow == ncol
    dim = min(nrow, ncol)
    if dim <= tiny_dense_threshold:
        return _dense_norm(B, herm)
    dev = storage_type(B).device
    eps = float(torch.finfo(T).eps)
    tol = math.sqrt(eps) if tol is None else float(tol)
    if herm:
        per_step = 1

        def step(w, v):
            mul(w, B, v)
    else:
        Bt = adjoint(B)
        per_step = 2
        if ncol <= nrow:                                                # B'B on vectors of length ncol
            tmp = torch.empty(nrow, dtype=T, device=dev)

            def step(w, v):
                mul(tmp, B, v)
                mul(w, Bt, tmp)
        else:                                                           # B B' on vectors of length nrow
            tmp = torch.empty(ncol, dtype=T, device=dev)

            def step(w, v):
                mul(tmp, Bt, v)
                mul(w, B, tmp)
    if ncv is None:
        ncv = max(20, 3) if herm else 10
    ncv = max(1, min(int(ncv), dim, 128))
    for attempt in range(max_attempts):
        L = _Lanczos(step, dim, ncv, T, dev)
        L.start(torch.randn(dim, dtype=T, device=dev, generator=generator))
        applies = 0
        while True:
            m = min(ncv, (maxiter - applies) // per_step)
            if m < 1:
                break
            alpha, beta = L.cycle(m)
            applies += m * per_step
            theta, y, residual, breakdown = lanczos_ritz(alpha, beta, dim, eps)
            if not math.isfinite(theta):
                break
            if breakdown is not None or residual <= tol * abs(theta):
                return (abs(theta) if herm else math.sqrt(max(theta, 0.0))), True
            if applies + per_step > maxiter:
                break
            L.restart(y)
        grown = min(2 * ncv, dim, 128)                                   # ext/LinearOperatorsOpNormExt.jl:73-81
        if grown <= ncv:
            break
        ncv = grown
    return math.nan, False
