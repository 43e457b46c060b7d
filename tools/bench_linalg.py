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

--block: the block right-hand sides instead, `mul!(R, op, V)` with V n x k for k = 2, 8, 32 at n = 2048, 8192, 16384 — time,
spread, launches and the model GB/s of FACTOR traffic (per group of 8 columns the factor is read once: n (n + 1) / 2 elements
for a triangular solve, twice that for Cholesky / LDLᵀ, n² for LU) — and beside each the loop of k single-vector applies in the
same run (the vector kernels, which the block form leaves untouched) and the vendor solve on the n x k block
(torch.cholesky_solve / torch.linalg.lu_solve / torch.linalg.solve_triangular; opLDL has the Cholesky one as yardstick). The
k = 1 rows are the single-vector applies. --mul-only prints the `mul!(R, op, V)` column alone (the protocol for a baseline
run of the same shapes on another commit).

    python tools/bench_linalg.py --block [n ...] > profiles/linalg_block.txt

--refine: the apply of opCholesky, opLDL, opLU and transpose(opLU) built with refine = 0, 1, 2, at n = 2048, 8192, 16384 in both
precisions, for k = 1 and k = 8: time, spread, launches, and the fraction of the 8 TB/s peak by the byte model of DESIGN.md §4
((r + 1) reads of the factor and r n² elements for the residuals per group). `x r=0` is the time over the refine = 0 row;
the expectation to hold it against is (r + 1) + r × (residual time / plain apply time). The refine = 0 rows are the plain apply;
the same shapes on another commit come from `--block --mul-only` (its k = 1 and k = 8 rows), which is how a baseline is taken.

    python tools/bench_linalg.py --refine [n ...] > profiles/linalg_refine.txt

--qr: opQR on a tall-thin (10⁶ x 128) and a square (8192²) Gaussian matrix (the square one with √n on its diagonal), both
precisions: the factorisation (construction, allocations and the one synchronisation included) and the apply in both modes —
time, spread, launches, and the fraction of the 8 TB/s peak by the byte model (mf·nf + nf²/2)·sizeof(T) — and, for comparison,
what a caller had to do before: opCholesky(AᵀA) (the Gram matrix by a torch GEMM) and per apply the dense Aᵀv plus the
Cholesky apply. The k = 8 and k = 32 rows are `mul!(X, op, V)` on a matrix operand in both modes, rated by the block's byte
model: the factor once per group of 8 columns, ⌈k/8⌉·(mf·nf + nf²/2)·sizeof(T), plus the operands, (mf + nf)·k·sizeof(T).
--mul-only prints the apply rows alone (the protocol for a baseline run on another commit). Other shapes: arguments of the
form MFxNF.

    python tools/bench_linalg.py --qr [MFxNF ...] > profiles/linalg_qr.txt

--qrp: opQR(A, pivot=True) on the matrices of --qr, each row beside the unpivoted one of the same run: the factorisation (rated
by its byte model, 2·sizeof(T)·Σ_c (mf − c)(nf − c)) and the vector apply in both modes at rank nf, where the two run the same
kernels; the last column is the time over the unpivoted row's.

    python tools/bench_linalg.py --qrp [MFxNF ...] > profiles/linalg_qrp.txt

--pinv: opPinv(A) beside opQR(A, pivot=True) of the same matrix in the same run, on the matrices of --qr made rank-deficient: the
last quarter of the columns is replaced by Gaussian combinations of the others (rank 3 nf / 4). The construction of both, and
the apply in both modes on a vector and on k = 8 columns; GB/s by the two-read models — 2·mf·r·sizeof(T) for the basic apply,
2·(mf + nf)·r·sizeof(T) for opPinv's —, the last column the time over the pivoted row's, to be held against 1 + nf/mf.

    python tools/bench_linalg.py --pinv [MFxNF ...] > profiles/linalg_pinv.txt

--ldlp: opLDL(K, pivot=True) on the indefinite K = (G + Gᵀ)/√(2n) at n = 2048, 8192, 16384 in both precisions: the factorisation
(construction, allocations and the one synchronisation included) and the apply on a vector, on k = 8 columns and as a graph
replay — and, in the same run, the yardsticks: opLU(K), what a caller had for such a matrix before; the unpivoted opLDL on a
quasi-definite matrix of the same n, which prices the pivoting; torch.linalg.ldl_factor / ldl_solve on the device where this
torch has them (n <= 2048 only: the vendor factorisation takes 52 s at n = 8192). GB/s by the byte model of two reads of the triangle (n² elements for opLU). `x opLU` is the time over the opLU
row of the same kind. `--ldlp --once n` builds one Float64 opLDL(K, pivot=True) and one opLU(K) and nothing else: the run to put
under a kernel trace, whose per-kernel totals are the panel's share of the factorisation.

    python tools/bench_linalg.py --ldlp [n ...] > profiles/linalg_ldlp.txt
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
BLOCK = "--block" in sys.argv
MUL_ONLY = "--mul-only" in sys.argv
REFINE = "--refine" in sys.argv
LDLP = "--ldlp" in sys.argv
VENDOR_MAX = 2048      # --ldlp: the largest n at which torch.linalg.ldl_factor on the device is timed
NS = [int(a) for a in sys.argv[1:] if not a.startswith("--") and "x" not in a] or ([2048, 8192, 16384] if BLOCK or REFINE or LDLP else [1024, 4096, 16384])


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


def colmajor(n, k, dtype, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(k, n, dtype=dtype, device=dev, generator=gen).t()


def block_legs():
    """mul!(R, op, V) on n x k blocks: see the module docstring"""
    print(f"# {torch.cuda.get_device_name(0)}; block right-hand sides; ms per call, median of 3 event-timed windows, spread = (max - min) / median")
    print(f"# GB/s: factor bytes of the model (one read per group of 8 columns) / time of mul!(R, op, V)")
    print(f"{'case':30s} {'n':>6s} {'k':>3s} {'mul ms':>9s} {'spread':>6s} {'launch':>6s} {'GB/s':>8s} | {'k applies':>9s} {'spread':>6s} {'launch':>6s} {'ratio':>6s} | "
          f"{'torch ms':>9s} {'ratio':>6s}", flush=True)
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        es = 8 if dtype is torch.float64 else 4
        for n in NS:
            M = spd(n, dtype)
            tri, full = n * (n + 1) // 2 * es, n * n * es
            reps = 20 if n <= 2048 else (5 if n <= 8192 else 3)
            Lt = torch.linalg.cholesky(M)
            Lc = Lt.t().contiguous().t()
            A = simple_matrix(n, dtype)
            LUt, pivt = torch.linalg.lu_factor(A)
            inv = lo.opInverse(Lc)
            lu = lo.opLU(A)
            cases = [("opCholesky", lo.opCholesky(M), 2 * tri, lambda V: torch.cholesky_solve(V, Lt)),
                     ("opLDL", lo.opLDL(quasi_definite(M)), 2 * tri, None),
                     ("opInverse(L)", inv, tri, lambda V: torch.linalg.solve_triangular(Lc, V, upper=False)),
                     ("transpose(opInverse(L))", inv.T, tri, lambda V: torch.linalg.solve_triangular(Lc.t(), V, upper=True)),
                     ("opLU", lu, full, lambda V: torch.linalg.lu_solve(LUt, pivt, V)),
                     ("transpose(opLU)", lu.T, full, lambda V: torch.linalg.lu_solve(LUt, pivt, V, adjoint=True))]
            for name, op, fbytes, tfn in cases:
                for k in (1, 2, 8, 32):
                    V, R = colmajor(n, k, dtype, 10 * n + k), colmajor(n, k, dtype, 1)
                    if k == 1:
                        v, r = V[:, 0], R[:, 0]
                        mul = lambda: lo.mul(r, op, v, 1.0, 0.0)
                    else:
                        mul = lambda: lo.mul(R, op, V, 1.0, 0.0)

                    def loop():
                        for j in range(k):
                            lo.mul(R[:, j], op, V[:, j], 1.0, 0.0)

                    ms = timeit(mul, reps)
                    sp, nl = timeit.spread, launches(mul)
                    gbs = -(-k // 8) * fbytes / ms / 1e6
                    line = f"{name + ' ' + tag:30s} {n:6d} {k:3d} {ms:9.4f} {100 * sp:5.1f}% {nl:6d} {gbs:8.1f} | "
                    if MUL_ONLY:
                        print(line, flush=True)
                        continue
                    lms = timeit(loop, reps) if k > 1 else ms
                    lsp, ll = timeit.spread, launches(loop)
                    tms = timeit(lambda: tfn(V), reps) if tfn else float("nan")
                    print(line + f"{lms:9.4f} {100 * lsp:5.1f}% {ll:6d} {lms / ms:6.2f} | {tms:9.4f} {tms / ms:6.2f}", flush=True)
            del cases, inv, lu, M, Lt, Lc, A, LUt, pivt
            torch.cuda.empty_cache()


def refine_legs():
    """the apply with refine = 0, 1, 2: see the module docstring"""
    print(f"# {torch.cuda.get_device_name(0)}; iterative refinement; ms per call, median of 3 event-timed windows, spread = (max - min) / median")
    print(f"# bytes: (r + 1) reads of the factor + r n^2 elements for the residuals, per group of 8 columns; peak {PEAK:.0f} GB/s")
    print(f"{'case':26s} {'n':>6s} {'k':>2s} {'r':>2s} {'ms':>9s} {'spread':>6s} {'launch':>6s} {'GB/s':>8s} {'%peak':>6s} {'x r=0':>6s}", flush=True)
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        es = 8 if dtype is torch.float64 else 4
        for n in NS:
            M = spd(n, dtype)
            K = quasi_definite(M)
            A = simple_matrix(n, dtype)
            tri, full = n * (n + 1) // 2 * es, n * n * es
            reps = 20 if n <= 2048 else (5 if n <= 8192 else 3)
            for name, make, X, fbytes, tr in (("opCholesky", lo.opCholesky, M, 2 * tri, False), ("opLDL", lo.opLDL, K, 2 * tri, False),
                                              ("opLU", lo.opLU, A, full, False), ("transpose(opLU)", lo.opLU, A, full, True)):
                base = {}
                for r in (0, 1, 2):
                    op = make(X, refine=r)
                    op = op.T if tr else op
                    for k in (1, 8):
                        V, R = colmajor(n, k, dtype, 10 * n + k), colmajor(n, k, dtype, 1)
                        v, res = (V[:, 0], R[:, 0]) if k == 1 else (V, R)
                        mul = lambda: lo.mul(res, op, v, 1.0, 0.0)
                        ms = timeit(mul, reps)
                        sp, nl = timeit.spread, launches(mul)
                        base.setdefault(k, ms)
                        gbs = ((r + 1) * fbytes + r * full) / ms / 1e6
                        print(f"{name + ' ' + tag:26s} {n:6d} {k:2d} {r:2d} {ms:9.4f} {100 * sp:5.1f}% {nl:6d} {gbs:8.1f} {100 * gbs / PEAK:6.2f} "
                              f"{ms / base[k]:6.2f}", flush=True)
                    del op
                    torch.cuda.empty_cache()
            del M, K, A
            torch.cuda.empty_cache()


def qr_legs():
    """opQR: see the module docstring"""
    print(f"# {torch.cuda.get_device_name(0)}; opQR; ms per call, median of 3 event-timed windows, spread = (max - min) / median")
    print(f"# bytes of an apply: (mf nf + nf^2 / 2) sizeof(T); peak {PEAK:.0f} GB/s. normal equations: opCholesky(A'A) built from a "
          f"torch GEMM, apply = dense A'v (LinearOperatorFromMatrix) + opCholesky apply")
    print(f"{'case':44s} {'mf':>8s} {'nf':>5s} {'ms':>10s} {'spread':>6s} {'launch':>6s} {'GB/s':>8s} {'%peak':>6s}", flush=True)
    shapes = [tuple(int(x) for x in a.split("x")) for a in sys.argv[1:] if "x" in a] or [(1000000, 128), (8192, 8192)]
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        es = 8 if dtype is torch.float64 else 4
        for mf, nf in shapes:
            gen = torch.Generator(device=dev).manual_seed(mf + nf)
            A = torch.randn(nf, mf, dtype=dtype, device=dev, generator=gen).t()           # column-major mf x nf
            if mf == nf:
                A = A + (nf ** 0.5) * torch.eye(nf, dtype=dtype, device=dev)
            v = torch.randn(mf, dtype=dtype, device=dev, generator=gen)
            u = torch.randn(nf, dtype=dtype, device=dev, generator=gen)
            x, y = torch.empty_like(u), torch.empty_like(v)
            nbytes = (mf * nf + nf * nf // 2) * es
            reps = 10 if mf * nf <= 2 ** 27 else 5

            def row(name, fn, reps, nbytes, nl):
                ms = timeit(fn, reps)
                gbs = nbytes / ms / 1e6 if nbytes else 0.0
                print(f"{name + ' ' + tag:44s} {mf:8d} {nf:5d} {ms:10.4f} {100 * timeit.spread:5.1f}% {nl:6d} {gbs:8.1f} {100 * gbs / PEAK:6.2f}",
                      flush=True)

            if not MUL_ONLY:
                row("opQR(A) factorisation", lambda: lo.opQR(A), 2, 0, 0)
            op = lo.opQR(A)
            row("opQR apply (least squares)", lambda: lo.mul(x, op, v, 1.0, 0.0), reps, nbytes, launches(lambda: lo.mul(x, op, v, 1.0, 0.0)))
            row("transpose(opQR) apply (minimum norm)", lambda: lo.mul(y, op.T, u, 1.0, 0.0), reps, nbytes,
                launches(lambda: lo.mul(y, op.T, u, 1.0, 0.0)))
            for k in (8, 32):                           # matrix operands: the factor once per group of 8 columns, plus the operands
                V, U = colmajor(mf, k, dtype, 10 * mf + k), colmajor(nf, k, dtype, 10 * nf + k)
                X, Y = torch.empty_like(U), torch.empty_like(V)
                kbytes = -(-k // 8) * nbytes + (mf + nf) * k * es
                kreps = max(2, reps // (k // 8))
                row(f"opQR apply, k = {k}", lambda: lo.mul(X, op, V, 1.0, 0.0), kreps, kbytes, launches(lambda: lo.mul(X, op, V, 1.0, 0.0)))
                row(f"transpose(opQR) apply, k = {k}", lambda: lo.mul(Y, op.T, U, 1.0, 0.0), kreps, kbytes,
                    launches(lambda: lo.mul(Y, op.T, U, 1.0, 0.0)))
                del V, U, X, Y
            del op
            torch.cuda.empty_cache()
            if MUL_ONLY:
                del A
                continue
            dense = lo.LinearOperatorFromMatrix(A)
            t = torch.empty_like(u)
            row("normal equations: A'A + opCholesky", lambda: lo.opCholesky((A.t() @ A).t().contiguous().t()), 2, 0, 0)
            ch = lo.opCholesky((A.t() @ A).t().contiguous().t())

            def normal():
                lo.mul(t, dense.T, v, 1.0, 0.0)
                lo.mul(x, ch, t, 1.0, 0.0)

            row("normal equations: A'v + opCholesky apply", normal, reps, (mf * nf + nf * nf) * es, launches(normal))
            del ch, dense, A
            torch.cuda.empty_cache()


def qrp_legs():
    """opQR(A, pivot=True) beside opQR(A) in the same run: see the module docstring"""
    print(f"# {torch.cuda.get_device_name(0)}; opQR(A, pivot=True) beside opQR(A); ms per call, median of 3 event-timed windows, "
          f"spread = (max - min) / median")
    print(f"# factorisation: construction, allocations and the one synchronisation included; model bytes of the pivoted one: "
          f"2 sizeof(T) sum_c (mf - c)(nf - c). apply: (mf nf + nf^2 / 2) sizeof(T), at rank nf; peak {PEAK:.0f} GB/s")
    print(f"{'case':44s} {'mf':>8s} {'nf':>5s} {'ms':>10s} {'spread':>6s} {'launch':>6s} {'GB/s':>8s} {'%peak':>6s} {'x plain':>8s}", flush=True)
    shapes = [tuple(int(x) for x in a.split("x")) for a in sys.argv[1:] if "x" in a] or [(1000000, 128), (8192, 8192)]
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        es = 8 if dtype is torch.float64 else 4
        for mf, nf in shapes:
            gen = torch.Generator(device=dev).manual_seed(mf + nf)
            A = torch.randn(nf, mf, dtype=dtype, device=dev, generator=gen).t()           # the matrices of --qr
            if mf == nf:
                A = A + (nf ** 0.5) * torch.eye(nf, dtype=dtype, device=dev)
            v = torch.randn(mf, dtype=dtype, device=dev, generator=gen)
            u = torch.randn(nf, dtype=dtype, device=dev, generator=gen)
            x, y = torch.empty_like(u), torch.empty_like(v)
            nbytes = (mf * nf + nf * nf // 2) * es
            fbytes = 2 * es * sum((mf - c) * (nf - c) for c in range(nf))
            reps = 10 if mf * nf <= 2 ** 27 else 5
            base = {}

            def row(name, fn, reps, nbytes, nl, key=None):
                ms = timeit(fn, reps)
                gbs = nbytes / ms / 1e6 if nbytes else 0.0
                ratio = f"{ms / base[key]:8.3f}" if key in base else f"{'':8s}"
                base.setdefault(key, ms)
                print(f"{name + ' ' + tag:44s} {mf:8d} {nf:5d} {ms:10.4f} {100 * timeit.spread:5.1f}% {nl:6d} {gbs:8.1f} {100 * gbs / PEAK:6.2f} "
                      f"{ratio}", flush=True)

            row("opQR(A) factorisation", lambda: lo.opQR(A), 1, 0, 0, "f")
            row("opQR(A, pivot=True) factorisation", lambda: lo.opQR(A, pivot=True), 1, fbytes, 0, "f")
            plain, piv = lo.opQR(A), lo.opQR(A, pivot=True)
            assert piv._rank == nf, piv._rank
            for name, res, w, wp, rhs, key in (("apply (least squares)", x, plain, piv, v, "n"),
                                               ("transposed apply (minimum norm)", y, plain.T, piv.T, u, "t")):
                row("opQR " + name, lambda: lo.mul(res, w, rhs, 1.0, 0.0), reps, nbytes, launches(lambda: lo.mul(res, w, rhs, 1.0, 0.0)), key)
                row("pivoted " + name, lambda: lo.mul(res, wp, rhs, 1.0, 0.0), reps, nbytes,
                    launches(lambda: lo.mul(res, wp, rhs, 1.0, 0.0)), key)
            del plain, piv, A
            torch.cuda.empty_cache()


def pinv_legs():
    """opPinv(A) beside opQR(A, pivot=True) on rank-deficient matrices: see the module docstring"""
    print(f"# {torch.cuda.get_device_name(0)}; opPinv(A) beside opQR(A, pivot=True), rank 3 nf / 4; ms per call, median of 3 event-timed "
          f"windows, spread = (max - min) / median")
    print(f"# construction: allocations and the synchronisations included. apply: two reads of the panels, 2 mf r sizeof(T) (basic) and "
          f"2 (mf + nf) r sizeof(T) (opPinv), per group of 8 columns; peak {PEAK:.0f} GB/s; x pivoted: to be held against 1 + nf/mf")
    print(f"{'case':44s} {'mf':>8s} {'nf':>5s} {'rank':>5s} {'k':>2s} {'ms':>10s} {'spread':>6s} {'launch':>6s} {'GB/s':>8s} {'%peak':>6s} "
          f"{'x pivoted':>9s} {'1+nf/mf':>8s}", flush=True)
    shapes = [tuple(int(x) for x in a.split("x")) for a in sys.argv[1:] if "x" in a] or [(1000000, 128), (8192, 8192)]
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        es = 8 if dtype is torch.float64 else 4
        for mf, nf in shapes:
            gen = torch.Generator(device=dev).manual_seed(mf + nf)
            A = torch.randn(nf, mf, dtype=dtype, device=dev, generator=gen).t()           # the matrices of --qr
            if mf == nf:
                A = A + (nf ** 0.5) * torch.eye(nf, dtype=dtype, device=dev)
            keep = nf - nf // 4
            comb = torch.randn(keep, nf - keep, dtype=dtype, device=dev, generator=gen) / keep ** 0.5
            A[:, keep:] = A[:, :keep] @ comb
            reps = 10 if mf * nf <= 2 ** 27 else 5
            base = {}

            def row(name, fn, reps, nbytes, nl, key, r, k):
                ms = timeit(fn, reps)
                gbs = nbytes / ms / 1e6 if nbytes else 0.0
                ratio = f"{ms / base[key]:9.3f} {1 + nf / mf:8.4f}" if key in base else f"{'':9s} {'':8s}"
                base.setdefault(key, ms)
                print(f"{name + ' ' + tag:44s} {mf:8d} {nf:5d} {r:5d} {k:2d} {ms:10.4f} {100 * timeit.spread:5.1f}% {nl:6d} {gbs:8.1f} "
                      f"{100 * gbs / PEAK:6.2f} {ratio}", flush=True)

            piv, pin = lo.opQR(A, pivot=True), lo.opPinv(A)
            r = pin._rank
            assert piv._rank == r and r < nf and len(pin._factor) == 8, (piv._rank, r)
            row("opQR(A, pivot=True) construction", lambda: lo.opQR(A, pivot=True), 1, 0, 0, "f", r, 0)
            row("opPinv(A) construction", lambda: lo.opPinv(A), 1, 0, 0, "f", r, 0)
            for k in (1, 8):
                v = colmajor(mf, k, dtype, 1)[:, 0] if k == 1 else colmajor(mf, k, dtype, 1)
                u = colmajor(nf, k, dtype, 2)[:, 0] if k == 1 else colmajor(nf, k, dtype, 2)
                x, y = torch.empty_like(u), torch.empty_like(v)
                for name, res, wp, wq, rhs in (("apply", x, piv, pin, v), ("transposed apply", y, piv.T, pin.T, u)):
                    key = (name, k)
                    row("pivoted " + name, lambda: lo.mul(res, wp, rhs, 1.0, 0.0), reps, 2 * mf * r * es,
                        launches(lambda: lo.mul(res, wp, rhs, 1.0, 0.0)), key, r, k)
                    row("opPinv " + name, lambda: lo.mul(res, wq, rhs, 1.0, 0.0), reps, 2 * (mf + nf) * r * es,
                        launches(lambda: lo.mul(res, wq, rhs, 1.0, 0.0)), key, r, k)
            del piv, pin, A
            torch.cuda.empty_cache()


def indefinite(n, dtype):
    """(G + G') / sqrt(2 n): the `indef` family of tests/ldl_pivot_cases.py, column-major"""
    gen = torch.Generator(device=dev).manual_seed(7700 + n)
    G = torch.randn(n, n, dtype=torch.float64, device=dev, generator=gen)
    return ((G + G.t()) / (2 * n) ** 0.5).to(dtype).t().contiguous().t()


def ldlp_legs():
    """opLDL(K, pivot=True) beside opLU(K), the unpivoted opLDL and the vendor's LDL': see the module docstring"""
    if "--once" in sys.argv:
        K = indefinite(NS[0], torch.float64)
        lo.opLDL(K, pivot=True)
        lo.opLU(K)
        torch.cuda.synchronize()
        return
    print(f"# {torch.cuda.get_device_name(0)}; opLDL(K, pivot=True) on K = (G + G') / sqrt(2 n); ms per call, median of 3 event-timed windows, "
          f"spread = (max - min) / median")
    print(f"# factorisation: construction, allocations and the one synchronisation included. apply: two reads of the triangle, n (n + 1) "
          f"sizeof(T) (opLU: n^2 sizeof(T)), per group of 8 columns; peak {PEAK:.0f} GB/s. unpivoted opLDL: on a quasi-definite matrix")
    print(f"{'case':46s} {'n':>6s} {'k':>2s} {'ms':>10s} {'spread':>6s} {'launch':>6s} {'GB/s':>8s} {'%peak':>6s} {'x opLU':>7s}", flush=True)
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        es = 8 if dtype is torch.float64 else 4
        for n in NS:
            K = indefinite(n, dtype)
            Q = quasi_definite(spd(n, dtype))
            tri2, full = n * (n + 1) * es, n * n * es
            reps = 20 if n <= 2048 else (5 if n <= 8192 else 3)
            base = {}

            def row(name, fn, reps, nbytes, nl, key, k):
                ms = timeit(fn, reps)
                gbs = nbytes / ms / 1e6 if nbytes else 0.0
                ratio = f"{ms / base[key]:7.3f}" if key in base else f"{'':7s}"
                if name.startswith("opLU"):
                    base[key] = ms
                print(f"{name + ' ' + tag:46s} {n:6d} {k:2d} {ms:10.4f} {100 * timeit.spread:5.1f}% {nl:6d} {gbs:8.1f} {100 * gbs / PEAK:6.2f} {ratio}",
                      flush=True)

            row("opLU(K) factorisation", lambda: lo.opLU(K), 1, 0, 0, "f", 0)
            row("opLDL(K, pivot=True) factorisation", lambda: lo.opLDL(K, pivot=True), 1, 0, 0, "f", 0)
            row("unpivoted opLDL(Q) factorisation", lambda: lo.opLDL(Q), 1, 0, 0, "f", 0)
            tsolve = None
            try:                                        # the vendor LDL' (pivoted), as far as this torch has it on the device, and only
                if n > VENDOR_MAX:                      # where it ends in reasonable time: it grows faster than n^3 (52 s at n = 8192)
                    raise RuntimeError(f"skipped for n > {VENDOR_MAX}")
                LD, piv = torch.linalg.ldl_factor(K)
                row("torch.linalg.ldl_factor(K)", lambda: torch.linalg.ldl_factor(K), 1, 0, 0, "f", 0)
                torch.linalg.ldl_solve(LD, piv, colmajor(n, 1, dtype, 3))
                tsolve = lambda V: torch.linalg.ldl_solve(LD, piv, V)
            except RuntimeError as err:
                print(f"# torch.linalg.ldl_factor / ldl_solve on the device: {str(err).splitlines()[0]}", flush=True)
            lu, piv_op, plain = lo.opLU(K), lo.opLDL(K, pivot=True), lo.opLDL(Q)
            for k in (1, 8):
                V, R = colmajor(n, k, dtype, 10 * n + k), colmajor(n, k, dtype, 1)
                v, res = (V[:, 0], R[:, 0]) if k == 1 else (V, R)
                for name, op, nbytes in (("opLU apply", lu, full), ("opLDL(pivot=True) apply", piv_op, tri2), ("unpivoted opLDL apply", plain, tri2)):
                    mul = lambda: lo.mul(res, op, v, 1.0, 0.0)
                    row(name, mul, reps, nbytes, launches(mul), ("a", k), k)
                if tsolve:
                    row("torch.linalg.ldl_solve", lambda: tsolve(V), reps, 0, 0, ("a", k), k)
            v, res = colmajor(n, 1, dtype, 5)[:, 0], colmajor(n, 1, dtype, 6)[:, 0]
            for name, op, nbytes in (("opLU apply (graph replay)", lu, full), ("opLDL(pivot=True) apply (graph replay)", piv_op, tri2)):
                gr = lo.capture_mul(res, op, v, 1.0, 0.0)
                row(name, gr.replay, reps, nbytes, 0, "g", 1)
                del gr
            del lu, piv_op, plain, K, Q, tsolve
            torch.cuda.empty_cache()


if LDLP:
    ldlp_legs()
    sys.exit(0)
if "--pinv" in sys.argv:
    pinv_legs()
    sys.exit(0)
if "--qrp" in sys.argv:
    qrp_legs()
    sys.exit(0)
if "--qr" in sys.argv:
    qr_legs()
    sys.exit(0)
if BLOCK:
    block_legs()
    sys.exit(0)
if REFINE:
    refine_legs()
    sys.exit(0)

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
