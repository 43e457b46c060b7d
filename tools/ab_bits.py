#!/usr/bin/env python
"""A/B of two builds of libmxlo.so by RESULT BITS: runs a fixed, seeded set of applies under the library named by
MXLO_LIB_PATH (default: the in-tree one) and prints one sha256 per case; `ab_bits.py --compare A.so B.so` runs itself
twice and reports the cases whose bits differ. Used when a kernel change claims "same summation tree, same bits"
(round 6: opHermitian's column butterfly off ds_bpermute; the push! passes; the dense block apply).

    gpurun -- 'python tools/ab_bits.py --compare tools/_ab/libmxlo_r05.so linearoperators.jl_amd/csrc/libmxlo.so herm'
"""
import hashlib
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def cases_herm(lo, torch, dev):
    for dt in (torch.float64, torch.float32):
        for n in (100, 256, 1000, 1024, 2048, 3000, 4096, 5000, 8192):
            g = torch.Generator(device="cpu").manual_seed(n)
            M = (torch.rand(n, n, dtype=dt, generator=g) - 0.5).to(dev).t()
            d, x, y = ((torch.rand(n, dtype=dt, generator=g) - 0.5).to(dev) for _ in range(3))
            H = lo.opHermitian(d, M)
            r = y.clone()
            lo.mul(r, H, x, 1.0, 0.0)
            yield f"herm {str(dt)[6:]} n={n} b0", r
            r = y.clone()
            lo.mul(r, H, x, 0.7, -1.3)
            yield f"herm {str(dt)[6:]} n={n} ab", r
            for k in (2, 3, 4, 7):
                V = (torch.rand(k, n, dtype=dt, generator=g) - 0.5).to(dev).t()
                R = torch.zeros(k, n, dtype=dt, device=dev).t()
                lo.mul(R, H, V, 1.0, 0.0)
                yield f"herm {str(dt)[6:]} n={n} block k={k}", R


def cases_dense(lo, torch, dev):
    for dt in (torch.float64, torch.float32):
        for (m, n) in ((1000, 700), (4096, 4096), (5000, 3000), (16384, 2048), (2048, 16384)):
            g = torch.Generator(device="cpu").manual_seed(m * 7 + n)
            M = (torch.rand(n, m, dtype=dt, generator=g) - 0.5).to(dev).t()
            op = lo.LinearOperatorFromMatrix(M)
            for k in (1, 2, 3, 4, 8, 11):
                V = (torch.rand(k, n, dtype=dt, generator=g) - 0.5).to(dev).t()
                R = (torch.rand(k, m, dtype=dt, generator=g) - 0.5).to(dev).t()
                if k == 1:
                    V, R = V[:, 0].contiguous(), R[:, 0].contiguous()
                r = R.clone()
                lo.mul(r, op, V, 1.0, 0.0)
                yield f"dense {str(dt)[6:]} {m}x{n} k={k} b0", r
                r = R.clone()
                lo.mul(r, op, V, 0.7, -1.3)
                yield f"dense {str(dt)[6:]} {m}x{n} k={k} ab", r
                U = (torch.rand(k, m, dtype=dt, generator=g) - 0.5).to(dev).t()
                Rt = torch.zeros(k, n, dtype=dt, device=dev).t()
                if k == 1:
                    U, Rt = U[:, 0].contiguous(), Rt[:, 0].contiguous()
                lo.mul(Rt, op.T, U, 1.0, 0.0)
                yield f"dense {str(dt)[6:]} {m}x{n} k={k} T", Rt


def cases_qn(lo, torch, dev):
    import numpy as np
    for dt in (torch.float64, torch.float32):
        for kind, ctor in (("inv", lo.InverseLBFGSOperator), ("fwd", lo.LBFGSOperator), ("sr1", lo.LSR1Operator)):
            for n, mem in ((1000, 5), (70001, 5), (1 << 20, 10), (3_000_017, 20)):
                rng = np.random.default_rng(n + mem)
                op = ctor(dt, n, mem=mem, device=dev)
                x = torch.from_numpy(rng.uniform(-1, 1, n)).to(dt).to(dev)
                for it in range(mem + 3):
                    s = torch.from_numpy(rng.uniform(-1, 1, n)).to(dt).to(dev)
                    yv = s * (1.0 + 0.5 * torch.from_numpy(rng.uniform(0, 1, n)).to(dt).to(dev))
                    if kind == "sr1":
                        yv = yv + 0.1 * torch.from_numpy(rng.uniform(-1, 1, n)).to(dt).to(dev)
                    lo.push(op, s, yv)
                r = torch.zeros(n, dtype=dt, device=dev)
                lo.mul(r, op, x, 1.0, 0.0)
                yield f"qn {kind} {str(dt)[6:]} n={n} m={mem} apply-after-pushes", r


def cases_persist(lo, torch, dev):
    """quasi-Newton applies in the range of the persistent single launch (qn.hip: qn_apply_persist_kernel), ragged lengths, alpha / beta / shift"""
    import numpy as np
    for dt in (torch.float64, torch.float32):
        for kind, ctor in (("inv", lo.InverseLBFGSOperator), ("fwd", lo.LBFGSOperator), ("sr1", lo.LSR1Operator)):
            for n, mem in (((1 << 19) + 5, 7), (1 << 19, 10), (700_001, 3), (1 << 20, 5), (1_500_001, 5), ((1 << 21) + 2, 10), (1 << 22, 5), (5_000_000, 4)):
                rng = np.random.default_rng(n + mem)
                op = ctor(dt, n, mem=mem, device=dev)
                x = torch.from_numpy(rng.uniform(-1, 1, n)).to(dt).to(dev)
                for it in range(mem + 2):
                    s = torch.from_numpy(rng.uniform(-1, 1, n)).to(dt).to(dev)
                    yv = s * (1.0 + 0.5 * torch.from_numpy(rng.uniform(0, 1, n)).to(dt).to(dev))
                    if kind == "sr1":
                        yv = yv + 0.1 * torch.from_numpy(rng.uniform(-1, 1, n)).to(dt).to(dev)
                    lo.push(op, s, yv)
                r = torch.from_numpy(rng.uniform(-1, 1, n)).to(dt).to(dev)
                lo.mul(r, op, x, 1.0, 0.0)
                yield f"persist {kind} {str(dt)[6:]} n={n} m={mem} b0", r
                lo.mul(r, op, x, 0.7, -1.3)
                yield f"persist {kind} {str(dt)[6:]} n={n} m={mem} ab", r
                del op


def cases_linalg(lo, torch, dev):
    """every apply of the factorisation operators (linalg.hip) at the smallest shapes that cross a block boundary (64), a group
    boundary (8 columns) and a rank deficiency: both modes, k = 1 (the vector entry points), 8, 9, beta = 0 and beta != 0"""
    def applies(tag, op, dt, g):
        for mode, o in (("N", op), ("T", op.T)):
            rows, cols = o.shape
            for k in (1, 8, 9):
                V = (torch.rand(k, cols, dtype=dt, generator=g) - 0.5).to(dev).t()
                R = (torch.rand(k, rows, dtype=dt, generator=g) - 0.5).to(dev).t()
                if k == 1:
                    V, R = V[:, 0].contiguous(), R[:, 0].contiguous()
                for name, a, b in (("b0", 1.0, 0.0), ("ab", 0.7, -0.75)):
                    r = R.clone()
                    lo.mul(r, o, V, a, b)
                    yield f"linalg {tag} {str(dt)[6:]} {mode} k={k} {name}", r

    for dt in (torch.float64, torch.float32):
        for n in (1, 64, 65, 200):
            g = torch.Generator(device="cpu").manual_seed(1000 + n)
            B = torch.rand(n, n, dtype=torch.float64, generator=g) - 0.5
            spd = (B @ B.t() + n * torch.eye(n, dtype=torch.float64)).to(dt)
            sym = (B + B.t() + torch.diag(torch.arange(1, n + 1, dtype=torch.float64) * (-1.0) ** torch.arange(n))).to(dt)
            gen = (B + 2.0 * torch.eye(n, dtype=torch.float64)).to(dt)
            col = lambda M: M.t().contiguous().to(dev).t()                          # column-major on the device
            for refine in (0, 2):
                yield from applies(f"opCholesky n={n} refine={refine}", lo.opCholesky(col(spd), refine=refine), dt, g)
                yield from applies(f"opLDL n={n} refine={refine}", lo.opLDL(col(sym), refine=refine), dt, g)
                yield from applies(f"opLU n={n} refine={refine}", lo.opLU(col(gen), refine=refine), dt, g)
            yield from applies(f"opLDL pivot n={n}", lo.opLDL(col(sym), pivot=True), dt, g)
            yield from applies(f"opLU row-major n={n}", lo.opLU(gen.contiguous().to(dev)), dt, g)
            yield from applies(f"opInverse lower n={n}", lo.opInverse(col(torch.tril(gen))), dt, g)
            yield from applies(f"opInverse upper n={n}", lo.opInverse(col(torch.triu(gen))), dt, g)
        for m, n, rank in ((5, 3, 2), (64, 64, 64), (129, 65, 64), (200, 129, 129), (200, 129, 65), (65, 200, 65)):
            g = torch.Generator(device="cpu").manual_seed(m * 1000 + n + rank)
            A = ((torch.rand(m, rank, dtype=torch.float64, generator=g) - 0.5) @
                 (torch.rand(rank, n, dtype=torch.float64, generator=g) - 0.5)).to(dt)
            for lay, Ad in (("col", A.t().contiguous().to(dev).t()), ("row", A.contiguous().to(dev))):
                tag = f"{m}x{n} r={rank} {lay}"
                if rank == min(m, n):
                    yield from applies(f"opQR {tag}", lo.opQR(Ad), dt, g)
                yield from applies(f"opQR pivot {tag}", lo.opQR(Ad, pivot=True), dt, g)
                yield from applies(f"opPinv {tag}", lo.opPinv(Ad), dt, g)


def cases_complex(lo, torch, dev):
    """complex.hip's dense leaves on ComplexF64 / ComplexF32: the GEMV in modes N, T, C and through the row-major alias at 1000x700,
    4096x1100 (row bands) and a view of 4096 rows at an odd offset and leading dimension (ComplexF32: column chunks); opHermitian with a
    real and a complex d under both cherm_two_pass values; beta = 0 and beta != 0 with res pre-filled"""
    ctx = lo.get_ctx(dev)
    scal = (("b0", complex(1), complex(0)), ("ab", 0.7 - 0.5j, -1.3 + 0.25j))

    def crand(g, rdt, *shape):
        return torch.complex(torch.rand(*shape, dtype=rdt, generator=g) - 0.5, torch.rand(*shape, dtype=rdt, generator=g) - 0.5)

    for dt, rdt in ((torch.complex128, torch.float64), (torch.complex64, torch.float32)):
        for tag, m, n, off in (("1000x700", 1000, 700, 0), ("4096x1100", 4096, 1100, 0), ("view 4096x1100", 4096, 1100, 1)):
            g = torch.Generator(device="cpu").manual_seed(m * 7 + n + off)
            big = crand(g, rdt, n, m + 3 * off).to(dev).t()                      # column-major, leading dimension m + 3 * off
            M = big[off:off + m, :]
            x, u, rm, rn = (crand(g, rdt, k).to(dev) for k in (n, m, m, n))
            ops = (("N", lo.LinearOperatorFromMatrix(M), x, rm), ("T", lo.LinearOperatorFromMatrix(M).T, u, rn),
                   ("C", lo.LinearOperatorFromMatrix(M).H, u, rn),
                   ("rowmajor N", lo.LinearOperatorFromMatrix(M.t()), u, rn), ("rowmajor C", lo.LinearOperatorFromMatrix(M.t()).H, x, rm))
            for mode, op, v, r0 in ops:
                for name, a, b in scal:
                    r = r0.clone()
                    lo.mul(r, op, v, a, b)
                    yield f"complex gemv {str(dt)[6:]} {tag} {mode} {name}", r
        for n in (100, 256, 1000, 1024, 3000):
            g = torch.Generator(device="cpu").manual_seed(n)
            A = crand(g, rdt, n, n).to(dev).t()
            x, y = crand(g, rdt, n).to(dev), crand(g, rdt, n).to(dev)
            for dname, d in (("real d", (torch.rand(n, dtype=rdt, generator=g) - 0.5).to(dev)), ("complex d", crand(g, rdt, n).to(dev))):
                H = lo.opHermitian(d, A)
                for two_pass in (0, 1):
                    with ctx.tuned(cherm_two_pass=two_pass):
                        for name, a, b in scal:
                            r = y.clone()
                            lo.mul(r, H, x, a, b)
                            yield f"complex herm {str(dt)[6:]} n={n} {dname} two_pass={two_pass} {name}", r


SECTIONS = {"herm": cases_herm, "dense": cases_dense, "qn": cases_qn, "persist": cases_persist, "linalg": cases_linalg,
            "complex": cases_complex}


def run(sections):
    import torch
    import __graft_entry__ as g
    lo = g.load_package()
    dev = torch.device("cuda", 0)
    for s in sections:
        for name, t in SECTIONS[s](lo, torch, dev):
            print(f"{digest(t)}  {name}", flush=True)


def compare(a, b, sections):
    outs = []
    for lib in (a, b):
        env = dict(os.environ, MXLO_LIB_PATH=os.path.abspath(lib))
        p = subprocess.run([sys.executable, os.path.abspath(__file__)] + sections, env=env, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"# run under {lib} failed (rc {p.returncode})")
            return 1
        outs.append({ln.split("  ", 1)[1]: ln.split("  ", 1)[0] for ln in p.stdout.splitlines() if "  " in ln})
    diff = [k for k in outs[0] if outs[0][k] != outs[1].get(k)]
    print(f"# {len(outs[0])} cases under A = {a} and B = {b}: {len(diff)} differ in bits")
    for k in diff:
        print(f"DIFF {k}: {outs[0][k]} vs {outs[1].get(k)}")
    return 1 if diff else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--compare":
        sys.exit(compare(args[1], args[2], args[3:] or list(SECTIONS)))
    run(args or list(SECTIONS))
