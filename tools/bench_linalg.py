#!/usr/bin/env python
"""opCholesky / opLDL / opLU / triangular opInverse on one MI355X: factorisation and apply times (HIP events after a warm-up), bytes
by the model of DESIGN.md §4 (one triangular solve reads the triangle once, n (n + 1) / 2 elements; a Cholesky or LDLᵀ apply
reads it twice, the latter 8 n bytes of pivots more), the fraction of the 8 TB/s peak, launches per apply — and next to
them the same solve through torch.cholesky_solve / torch.linalg.solve_triangular on the same device, which is what a
caller had to use before. The opLDL rows follow the opCholesky rows of the same n: the yardstick of opLDL is opCholesky in
the same run (torch column: torch.linalg.ldl_factor / ldl_solve, which pivot). Each time is the median of 3 windows; the
spread column is (max − min) / median of the three. The opLU rows (the simple_matrix of tests/test_gpu_lu.py at the same n,
U S V' with singular values 1 .. 2) have the opCholesky rows of the same n as their yardstick — the two applies are
the same number of launches over the same n² elements; torch column: torch.linalg.lu_factor / lu_solve.

    python tools/bench_linalg.py [n ...] > profiles/linalg_solve.txt
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import __graft_entry__ as g

lo = g.load_package()
from linearoperators_jl_amd.device import Timer, get_ctx

dev = torch.device("cuda", 0)
ctx = get_ctx(dev)
tm = Timer(ctx)
PEAK = 8000.0          # GB/s
NS = [int(a) for a in sys.argv[1:]] or [1024, 4096, 16384]


def timeit(fn, reps):
    """ms per call: the median of 3 windows of `reps` back-to-back calls between one pair of events, after a warm-up; the
    spread of the three windows is left in timeit.spread"""
    for _ in range(3):
        fn()
    out = []
    for _ in range(3):
        tm.start()
        for _ in range(reps):
            fn()
        tm.stop()
        out.append(tm.elapsed_ms() / reps)
    out.sort()
    timeit.spread = (out[2] - out[0]) / out[1] if out[1] else 0.0
    return out[1]


def launches(fn):
    a, b = (C.c_int64 * 12)(), (C.c_int64 * 12)()
    fn()
    lo._lib.call("mxlo_debug_counters", a)
    fn()
    lo._lib.call("mxlo_debug_counters", b)
    return b[10] - a[10]


def quasi_definite(M):
    """the signs of every third row and column flipped where both are: a symmetric permutation of [A B'; B -C]"""
    n = M.shape[0]
    neg = (torch.arange(n, device=dev) % 3 == 2)
    K = torch.where(neg[:, None] & neg[None, :], -M, M)
    return K.t().contiguous().t()


def spd(n, dtype):
    gen = torch.Generator(device=dev).manual_seed(n)
    G = torch.randn(n, n, dtype=torch.float64, device=dev, generator=gen) / n ** 0.5
    M = G @ G.t() + torch.eye(n, dtype=torch.float64, device=dev)
    return ((M + M.t()) / 2).to(dtype).t().contiguous().t()          # column-major


def simple_matrix(n, dtype):
    """the matrix of tests/test_gpu_lu.py (the reference's test/test_aux.jl:3-17): U S V' with singular values 1 .. 2"""
    gen = torch.Generator(device=dev).manual_seed(6200 + n)
    U = torch.linalg.qr(torch.rand(n, n, dtype=torch.float64, device=dev, generator=gen))[0]
    V = torch.linalg.qr(torch.rand(n, n, dtype=torch.float64, device=dev, generator=gen))[0]
    s = 1 + torch.arange(n, dtype=torch.float64, device=dev) / max(n - 1, 1)
    return ((U * s) @ V.t()).to(dtype).t().contiguous().t()


print(f"# {torch.cuda.get_device_name(0)}; times: ms per call, median of 3 event-timed windows; GB/s by the byte model; peak {PEAK:.0f} GB/s")
print(f"{'case':34s} {'n':>6s} {'ms':>9s} {'spread':>6s} {'GB/s':>8s} {'%peak':>6s} {'launch':>6s} | {'torch ms':>9s} {'ratio':>6s}")
for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
    es = 8 if dtype is torch.float64 else 4
    for n in NS:
        M = spd(n, dtype)
        v = torch.randn(n, dtype=dtype, device=dev)
        res = torch.empty_like(v)
        reps = 20 if n <= 4096 else 7
        tri = n * (n + 1) // 2 * es
        vec = 3 * n * es + 2 * n * 8 + (n + 63) // 64 * 4096 * 8      # v, res, the f64 work vector, the block inverses

        def row(name, fn, reps, nbytes, nl, tfn):
            ms = timeit(fn, reps)
            sp = timeit.spread
            tms = timeit(tfn, reps) if tfn else float("nan")
            gbs = nbytes / ms / 1e6 if nbytes else 0.0
            print(f"{name + ' ' + tag:34s} {n:6d} {ms:9.4f} {100 * sp:5.1f}% {gbs:8.1f} {100 * gbs / PEAK:6.2f} {nl:6d} | {tms:9.4f} {tms / ms:6.2f}")

        # factorisation (construction: allocations, the copy of the triangle and the one synchronisation included)
        freps = 5 if n <= 4096 else 3
        row("opCholesky(M) factorisation", lambda: lo.opCholesky(M), freps, 0, 0, lambda: torch.linalg.cholesky(M))
        K = quasi_definite(M)
        vt = v[:, None].clone()
        LD = piv = t_factor = t_solve = None                                          # the vendor LDLᵀ (pivoted), as far as this torch has it
        try:
            LD, piv = torch.linalg.ldl_factor(K)
            t_factor = lambda: torch.linalg.ldl_factor(K)
            torch.linalg.ldl_solve(LD, piv, vt)
            t_solve = lambda: torch.linalg.ldl_solve(LD, piv, vt)
        except RuntimeError:
            pass
        row("opLDL(K) factorisation", lambda: lo.opLDL(K), freps, 0, 0, t_factor)
        op = lo.opCholesky(M)
        ldl = lo.opLDL(K)
        Lt = torch.linalg.cholesky(M)
        row("opCholesky apply", lambda: lo.mul(res, op, v, 1.0, 0.0), reps, 2 * tri + vec,
            launches(lambda: lo.mul(res, op, v, 1.0, 0.0)), lambda: torch.cholesky_solve(vt, Lt))
        row("opLDL apply", lambda: lo.mul(res, ldl, v, 1.0, 0.0), reps, 2 * tri + vec + 8 * n,
            launches(lambda: lo.mul(res, ldl, v, 1.0, 0.0)), t_solve)
        Lc = Lt.t().contiguous().t()                                                  # column-major lower factor
        inv = lo.opInverse(Lc)
        row("opInverse(L) apply", lambda: lo.mul(res, inv, v, 1.0, 0.0), reps, tri + vec,
            launches(lambda: lo.mul(res, inv, v, 1.0, 0.0)), lambda: torch.linalg.solve_triangular(Lc, vt, upper=False))
        row("transpose(opInverse(L)) apply", lambda: lo.mul(res, inv.T, v, 1.0, 0.0), reps, tri + vec,
            launches(lambda: lo.mul(res, inv.T, v, 1.0, 0.0)), lambda: torch.linalg.solve_triangular(Lc.t(), vt, upper=True))
        gr = lo.capture_mul(res, op, v, 1.0, 0.0)                                     # the same apply replayed as one hipGraph
        row("opCholesky apply (graph replay)", gr.replay, reps, 2 * tri + vec, 0, lambda: torch.cholesky_solve(vt, Lt))
        gl = lo.capture_mul(res, ldl, v, 1.0, 0.0)
        row("opLDL apply (graph replay)", gl.replay, reps, 2 * tri + vec + 8 * n, 0, t_solve)
        A = simple_matrix(n, dtype)                                                   # general, column-major, condition number 2
        LUt, pivt = torch.linalg.lu_factor(A)
        row("opLU(A) factorisation", lambda: lo.opLU(A), freps, 0, 0, lambda: torch.linalg.lu_factor(A))
        lu = lo.opLU(A)
        full = n * n * es + 4 * n + (n + 63) // 64 * 4096 * 8                         # both triangles once each, perm, the second inverses
        row("opLU apply", lambda: lo.mul(res, lu, v, 1.0, 0.0), reps, full + vec,
            launches(lambda: lo.mul(res, lu, v, 1.0, 0.0)), lambda: torch.linalg.lu_solve(LUt, pivt, vt))
        row("transpose(opLU) apply", lambda: lo.mul(res, lu.T, v, 1.0, 0.0), reps, full + vec,
            launches(lambda: lo.mul(res, lu.T, v, 1.0, 0.0)), lambda: torch.linalg.lu_solve(LUt, pivt, vt, adjoint=True))
        del op, ldl, inv, gr, gl, M, K, Lt, Lc, LD, piv, A, LUt, pivt, lu
        torch.cuda.empty_cache()
