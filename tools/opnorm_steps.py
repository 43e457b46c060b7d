"""Measurements behind profiles/opnorm_steps.txt (run on an MI355X):
  * GB/s of mxlo_krylov_orth at n = 1e7, k in {5, 10, 20}, Float64, against the byte model of DESIGN.md §4
    ((4k + 6*ceil(k/10) + 2) * 8 B per element for the two unconditional rounds);
  * operator applies estimate_opnorm and normest need on an LBFGSOperator (n = 1e6, mem = 10) to agree with a tightly
    converged value to 1e-6.
Usage: python tools/opnorm_steps.py [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def orth_bandwidth(lo, dev, out, n=10_000_000, reps=20):
    ctx, L = lo.get_ctx(dev), lo._lib.lib()
    for k in (5, 10, 20):
        ldv = n + (-n) % 2
        basis = torch.randn((k + 1) * ldv, dtype=torch.float64, device=dev) / np.sqrt(n)     # near-orthonormal columns
        coef = torch.zeros(k + 1, dtype=torch.float64, device=dev)
        w = basis[k * ldv: k * ldv + n]
        model = (4 * k + 6 * -(-k // 10) + 2) * 8 * n
        for flags, label in ((0, "two rounds"), (1, "DGKS flag set")):
            times = []
            for r in range(reps + 3):
                w.normal_()
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                st = L.mxlo_krylov_orth(ctx.handle, 0, basis.data_ptr(), ldv, n, k, w.data_ptr(), coef.data_ptr(), flags)
                t1.record()
                torch.cuda.synchronize()
                assert st == 0
                if r >= 3:
                    times.append(t0.elapsed_time(t1))
            ms = statistics.median(times)
            print(f"mxlo_krylov_orth f64 n={n} k={k:2d} {label:14s}: median {ms:8.3f} ms (min {min(times):.3f}, max {max(times):.3f}, "
                  f"{reps} runs)  two-round byte model {model / 1e9:.2f} GB -> {model / ms / 1e6:7.1f} GB/s", file=out, flush=True)
        del basis


def apply_counts(lo, dev, out, n=1_000_000, mem=10):
    rng = np.random.default_rng(0)
    B = lo.LBFGSOperator(torch.float64, n, mem=mem, device=dev)
    T = lambda a: torch.from_numpy(a).to(dev)
    for i in range(mem + 3):
        s = rng.uniform(-1, 1, n)
        lo.push(B, T(s), T(s * rng.uniform(0.5, 2.0, n) + 1e-2 * rng.standard_normal(n)))
    count = [0]
    real_mul, real_apply = lo.opnorm.mul, lo.utilities.apply

    def mul(*a, **kw):
        count[0] += 1
        return real_mul(*a, **kw)

    def apply(*a, **kw):
        count[0] += 1
        return real_apply(*a, **kw)

    lo.opnorm.mul, lo.utilities.apply = mul, apply
    try:
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        ref, ok = lo.estimate_opnorm(B, tol=1e-10, generator=gen)
        print(f"LBFGSOperator n={n} mem={mem}: tightly converged value {ref!r} (tol 1e-10, converged {ok}, {count[0]} applies)", file=out)
        for tol in (1e-3, 1e-6, None):
            count[0] = 0
            gen.manual_seed(1)
            v, ok = lo.estimate_opnorm(B, tol=tol, generator=gen)
            print(f"  estimate_opnorm tol={tol}: {count[0]:4d} applies, value {v!r}, converged {ok}, |v - ref|/ref = {abs(v - ref) / ref:.2e}", file=out)
        for tol in (1e-3, 1e-6, 1e-8, 1e-10, 1e-12, 1e-14):
            count[0] = 0
            gen.manual_seed(1)
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                e, it = lo.normest(B, tol=tol, maxiter=2000, generator=gen)
            print(f"  normest tol={tol:g}: {count[0]:4d} applies ({it} iterations), value {e!r}, |e - ref|/ref = {abs(e - ref) / ref:.2e}", file=out, flush=True)
    finally:
        lo.opnorm.mul, lo.utilities.apply = real_mul, real_apply


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lo = g.load_package()
    dev = torch.device("cuda", 0)
    out = open(a.out, "w") if a.out else sys.stdout
    orth_bandwidth(lo, dev, out)
    apply_counts(lo, dev, out)
