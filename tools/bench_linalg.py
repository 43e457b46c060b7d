#!/usr/bin/env python
"""opCholesky / triangular opInverse on one MI355X: factorisation and apply times (HIP events after a warm-up), bytes by
the model of DESIGN.md §4 (one triangular solve reads the triangle once, n (n + 1) / 2 elements; a Cholesky apply reads it
twice), the fraction of the 8 TB/s peak, launches per apply — and next to them the same solve through
torch.cholesky_solve / torch.linalg.solve_triangular on the same device, which is what a caller had to use before.

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
    """ms per call: the median of 3 windows of `reps` back-to-back calls between one pair of events, after a warm-up"""
    for _ in range(3):
        fn()
    out = []
    for _ in range(3):
        tm.start()
        for _ in range(reps):
            fn()
        tm.stop()
        out.append(tm.elapsed_ms() / reps)
    return sorted(out)[1]


def launches(fn):
    a, b = (C.c_int64 * 12)(), (C.c_int64 * 12)()
    fn()
    lo._lib.call("mxlo_debug_counters", a)
    fn()
    lo._lib.call("mxlo_debug_counters", b)
    return b[10] - a[10]


def spd(n, dtype):
    gen = torch.Generator(device=dev).manual_seed(n)
    G = torch.randn(n, n, dtype=torch.float64, device=dev, generator=gen) / n ** 0.5
    M = G @ G.t() + torch.eye(n, dtype=torch.float64, device=dev)
    return ((M + M.t()) / 2).to(dtype).t().contiguous().t()          # column-major


print(f"# {torch.cuda.get_device_name(0)}; times: ms per call, median of 3 event-timed windows; GB/s by the byte model; peak {PEAK:.0f} GB/s")
print(f"{'case':34s} {'n':>6s} {'ms':>9s} {'GB/s':>8s} {'%peak':>6s} {'launch':>6s} | {'torch ms':>9s} {'ratio':>6s}")
for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
    es = 8 if dtype is torch.float64 else 4
    for n in NS:
        M = spd(n, dtype)
        v = torch.randn(n, dtype=dtype, device=dev)
        res = torch.empty_like(v)
        reps = 20 if n <= 4096 else 7
        tri = n * (n + 1) // 2 * es
        vec = 3 * n * es + 2 * n * 8 + (n + 63) // 64 * 4096 * 8      # v, res, the f64 work vector, the block inverses

        def row(name, ms, nbytes, nl, tms):
            gbs = nbytes / ms / 1e6 if nbytes else 0.0
            print(f"{name + ' ' + tag:34s} {n:6d} {ms:9.4f} {gbs:8.1f} {100 * gbs / PEAK:6.2f} {nl:6d} | {tms:9.4f} {tms / ms:6.2f}")

        # factorisation (construction: allocations, the copy of the triangle and the one synchronisation included)
        t_f = timeit(lambda: lo.opCholesky(M), 5 if n <= 4096 else 3)
        t_ft = timeit(lambda: torch.linalg.cholesky(M), 5 if n <= 4096 else 3)
        row("opCholesky(M) factorisation", t_f, 0, 0, t_ft)
        op = lo.opCholesky(M)
        Lt = torch.linalg.cholesky(M)
        vt = v[:, None].clone()
        row("opCholesky apply", timeit(lambda: lo.mul(res, op, v, 1.0, 0.0), reps), 2 * tri + vec,
            launches(lambda: lo.mul(res, op, v, 1.0, 0.0)), timeit(lambda: torch.cholesky_solve(vt, Lt), reps))
        Lc = Lt.t().contiguous().t()                                                  # column-major lower factor
        inv = lo.opInverse(Lc)
        row("opInverse(L) apply", timeit(lambda: lo.mul(res, inv, v, 1.0, 0.0), reps), tri + vec,
            launches(lambda: lo.mul(res, inv, v, 1.0, 0.0)),
            timeit(lambda: torch.linalg.solve_triangular(Lc, vt, upper=False), reps))
        row("transpose(opInverse(L)) apply", timeit(lambda: lo.mul(res, inv.T, v, 1.0, 0.0), reps), tri + vec,
            launches(lambda: lo.mul(res, inv.T, v, 1.0, 0.0)),
            timeit(lambda: torch.linalg.solve_triangular(Lc.t(), vt, upper=True), reps))
        gr = lo.capture_mul(res, op, v, 1.0, 0.0)                                     # the same apply replayed as one hipGraph
        row("opCholesky apply (graph replay)", timeit(gr.replay, reps), 2 * tri + vec, 0,
            timeit(lambda: torch.cholesky_solve(vt, Lt), reps))
        del op, inv, gr, M, Lt, Lc
        torch.cuda.empty_cache()
