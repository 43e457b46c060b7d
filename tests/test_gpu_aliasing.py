"""-m gpu: `mul!(x, op, x)` and overlapping windows of one buffer as res and v.

The reference defines these calls wherever its closure reads (or copies) all of v before it writes res:
  opDiagonal (square) and the diagonal quasi-Newton family  src/special-operators.jl:125-130   elementwise broadcast
  opHouseholder                                             src/linalg.jl:77-83                 dot(h, v) first
  opHermitian                                               src/linalg.jl:97-103                L*v, (v'*L)' materialised
  opRestriction (ranges, index lists, permutations)         src/special-operators.jl:167-169    broadcast unaliases view(v, I)
  kron(A, B)                                                src/kron.jl:14-40                   B*X*transpose(A) materialised
  InverseLBFGSOperator / LBFGSOperator                      src/lbfgs.jl:117-154, 173-202       q .= x first, res last
  op1 * op2                                                 src/operations.jl:117-128           through vtmp
  BlockDiagonalOperator of square opDiagonal / opEye        src/special-operators.jl:249-294    blocks on aligned views
Each case runs on separate buffers (checked against the oracle), then aliased — 3-arg, (2, 0), (0.75, -1.25), where with
beta != 0 the incoming res is v itself — and the aliased result must have the BITS of the separate-buffer one: the same
kernels in the same order, so one element a racing kernel corrupts fails the test. Windows: res = buf[s:], v = buf[:n]
and the reverse, against copies of both taken before the call (same alignments). Races depend on timing: every case
runs three times with fresh data, no more.

Out of scope — the reference's own aliased result is undefined or order-dependent there:
  LSR1Operator                      src/lsr1.jl:89-106 (res .= scaling_factor .* x, then reads x in the loop)
  op1 + op2                         src/operations.jl:188-196 (mul!(res, op1, v) writes res, then op2 reads v)
  hcat / vcat                       src/cat.jl (each block writes its view of res while later blocks read v)
  ShiftedOperator                   src/shifted_operators.jl:16-24 (axpy!(α*σ, x, res) after res was written)
  opExtension                       src/special-operators.jl:171-174 (res .= 0 first)
  dense and sparse LinearOperator(M)   behaviour of LinearAlgebra's mul!, not of the reference
  matrix / block applies, sharded paths
"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

NP = {torch.float64: np.float64, torch.float32: np.float32, torch.complex128: np.complex128}
SCAL = (None, (2.0, 0.0), (0.75, -1.25))          # None: the 3-arg form
SHIFTS = (1, 4, 257, 4097)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb else 1.0)


def launches(lo):
    a = (C.c_int64 * 12)()
    lo._lib.call("mxlo_debug_counters", a)
    return a[10]


def mul(lo, res, op, v, ab):
    if ab is None:
        lo.mul(res, op, v)
    else:
        lo.mul(res, op, v, *ab)
    return res


def rand(rng, n, dtype):
    if dtype.is_complex:
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(NP[dtype])
    return rng.uniform(-1, 1, n).astype(NP[dtype])


def check_aliased(lo, dev, op, v_h, dtype, oracle_fn=None, tol=None, one_launch=None):
    """Separate buffers vs the oracle, then mul!(x, op, x) bit-identical to the separate-buffer result.
    one_launch: the separate-buffer call is documented as one launch (asserted), and so is the aliased one."""
    for ab in SCAL:
        v = T(v_h, dev)
        res = v.clone()                                        # res0 = v: with beta != 0 the incoming res is v itself
        l0 = launches(lo)
        mul(lo, res, op, v, ab)
        if one_launch:
            assert launches(lo) - l0 == 1, ab
        if oracle_fn is not None:
            want = oracle_fn(v_h.copy(), ab)
            got = res.cpu().numpy()
            if tol == 0:
                assert np.array_equal(got, want), ab
            else:
                assert rel(got, want) <= tol, (ab, rel(got, want))
        x = v.clone()
        l0 = launches(lo)
        mul(lo, x, op, x, ab)
        if one_launch:
            assert launches(lo) - l0 == 1, ab
        torch.cuda.synchronize()
        bad = (x != res) & ~(torch.isnan(x) & torch.isnan(res))
        assert not bad.any(), (ab, int(bad.nonzero()[0]), int(bad.sum()))


def check_windows(lo, dev, op, n, nres, dtype, rng, shifts=SHIFTS):
    """res = buf[s:s+nres], v = buf[:n] and res = buf[:nres], v = buf[s:s+n]: bit-identical to the same call on copies of
    both windows taken before it (placed at the same offsets, so every alignment-dependent path is the same)."""
    for s in shifts:
        buf_h = rand(rng, max(n, nres) + s, dtype)
        for res_first in (False, True):
            rs, vs = (slice(0, nres), slice(s, s + n)) if res_first else (slice(s, s + nres), slice(0, n))
            for ab in SCAL[1:]:
                buf = T(buf_h, dev)
                want = T(buf_h, dev)[rs]
                mul(lo, want, op, T(buf_h, dev)[vs], ab)
                got = buf[rs]
                mul(lo, got, op, buf[vs], ab)
                torch.cuda.synchronize()
                bad = got != want
                assert not bad.any(), (s, res_first, ab, int(bad.nonzero()[0]), int(bad.sum()))


def ab_of(ab, dtype):
    return (1.0, 0.0) if ab is None else ab


# ------------------------------------------------------------------------------------------------ elementwise leaves
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", [1000, 3_000_001])
def test_diagonal(lo, dev, dtype, n):
    for rep in range(3):
        rng = np.random.default_rng(100 * rep + n % 97)
        d = rand(rng, n + 4097, dtype)
        D = lo.opDiagonal(T(d[:n], dev))
        check_aliased(lo, dev, D, rand(rng, n, dtype), dtype,
                      lambda v, ab: oracle.diag_mul(v.copy(), d[:n], v, *ab_of(ab, dtype),
                                                    flags=oracle.scalar_flags(NP[dtype], *ab_of(ab, dtype))), tol=0)
        check_windows(lo, dev, D, n, n, dtype, rng)


@pytest.mark.parametrize("kind", ["psb", "andrei", "bfgs"])
def test_diagonal_quasi_newton(lo, dev, kind):
    n = 1_000_003
    ctor = {"psb": lo.DiagonalPSB, "andrei": lo.DiagonalAndrei, "bfgs": lo.DiagonalBFGS}[kind]
    for rep in range(3):
        rng = np.random.default_rng(7 + rep)
        B = ctor(T(rng.uniform(0.5, 2.0, n), dev))
        s = rng.uniform(-1, 1, n)
        lo.push(B, T(s, dev), T(s * rng.uniform(0.5, 2.0, n), dev))
        d = B.d.cpu().numpy()
        check_aliased(lo, dev, B, rng.uniform(-1, 1, n), torch.float64,
                      lambda v, ab: oracle.diag_mul(v.copy(), d, v, *ab_of(ab, torch.float64)), tol=0)
        check_windows(lo, dev, B, n, n, torch.float64, rng)


def test_block_diagonal_of_diagonal_and_eye(lo, dev):
    n1, n2, n3 = 97_657, 250_001, 3
    for rep in range(3):
        rng = np.random.default_rng(11 + rep)
        d1, d3 = rng.uniform(-1, 1, n1), rng.uniform(-1, 1, n3)
        op = lo.BlockDiagonalOperator(lo.opDiagonal(T(d1, dev)), lo.opEye(torch.float64, n2, S=lo.Storage(torch.float64, dev)),
                                      lo.opDiagonal(T(d3, dev)))
        d = np.concatenate([d1, np.ones(n2), d3])
        n = n1 + n2 + n3
        check_aliased(lo, dev, op, rng.uniform(-1, 1, n), torch.float64,
                      lambda v, ab: oracle.diag_mul(v.copy(), d, v, *ab_of(ab, torch.float64)), tol=0)
        check_windows(lo, dev, op, n, n, torch.float64, rng, shifts=(1, 257))


# ------------------------------------------------------------------------------------------------ opHouseholder
HOUSE_TOL = {torch.float64: 1e-12, torch.float32: 1e-5, torch.complex128: 1e-12}
HOUSE_CASES = [(dt, n, f) for dt in HOUSE_TOL for n in (1000, 3_000_001) for f in (1, 0)] + \
              [(torch.float64, 30_000_000, 1), (torch.complex128, 30_000_000, 1)]     # n > 2^22 doubles: two passes


@pytest.mark.parametrize("dtype,n,fused", HOUSE_CASES)
def test_householder(lo, dev, dtype, n, fused):
    tol = HOUSE_TOL[dtype]
    ctx = lo.get_ctx(dev)
    with ctx.tuned(house_fused=fused):
        for rep in range(3):
            rng = np.random.default_rng(n % 1009 + rep)
            h = rand(rng, n, dtype)
            h /= np.linalg.norm(h)
            H = lo.opHouseholder(T(h, dev))

            def want(v, ab):
                a, b = ab_of(ab, dtype)
                if dtype.is_complex:
                    return a * (v - 2 * h * np.vdot(h, v)) + b * v
                return oracle.householder_mul(v.copy(), h, v, a, b, flags=oracle.scalar_flags(NP[dtype], a, b))
            one = fused == 1 and n == 3_000_001 and dtype == torch.float64
            check_aliased(lo, dev, H, rand(rng, n, dtype), dtype, want, tol, one_launch=one)
            check_aliased(lo, dev, H.H, rand(rng, n, dtype), dtype, want, tol)
            if dtype != torch.complex128 and n != 30_000_000:
                check_windows(lo, dev, H, n, n, dtype, rng)
        if n == 30_000_000 and dtype == torch.float64:
            check_windows(lo, dev, H, n, n, dtype, rng, shifts=(1, 4097))


# ------------------------------------------------------------------------------------------------ opHermitian
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.complex128, 1e-12)])
@pytest.mark.parametrize("n", [4096, 4099, 6144])
@pytest.mark.parametrize("single", [1, 0])
def test_hermitian(lo, dev, dtype, tol, n, single):
    ctx = lo.get_ctx(dev)
    with ctx.tuned(herm_single=single):
        for rep in range(3):
            rng = np.random.default_rng(n + rep)
            A = rand(rng, n * n, dtype).reshape(n, n)
            d = rng.uniform(-1, 1, n).astype(NP[dtype])
            Hm = lo.opHermitian(T(d, dev), torch.from_numpy(np.ascontiguousarray(A.T)).to(dev).t())

            def want(v, ab):
                a, b = ab_of(ab, dtype)
                return oracle.hermitian_mul(v.copy(), d, A, v, a, b)
            check_aliased(lo, dev, Hm, rand(rng, n, dtype), dtype, want, tol)


# ------------------------------------------------------------------------------------------------ opRestriction
@pytest.mark.parametrize("form", ["reverse_range", "permutation", "sorted_plan", "unit_range"])
def test_restriction(lo, dev, form):
    n = 1_000_000
    for rep in range(3):
        rng = np.random.default_rng(31 + rep)
        if form == "reverse_range":
            I, idx = lo.leaves.jrange(n, 1, -1), np.arange(n, 0, -1)
        elif form == "unit_range":
            I, idx = lo.leaves.jrange(1, n - 4097), np.arange(1, n - 4096)
        elif form == "permutation":
            idx = rng.permutation(n) + 1
            I = idx
        else:
            idx = np.sort(rng.choice(n, n // 2, replace=False)) + 1
            I = idx
        P = lo.opRestriction(I, n, device=dev)
        nres = idx.size
        v_h = rng.uniform(-1, 1, n)
        # separate buffers, bit-exact against v[I] (src/special-operators.jl:167-169: alpha, beta ignored)
        want = T(v_h[idx - 1], dev)
        got = torch.empty(nres, dtype=torch.float64, device=dev)
        lo.mul(got, P, T(v_h, dev))
        assert torch.equal(got, want)
        # res a prefix window of v (res == v for the square forms)
        buf = T(v_h, dev)
        lo.mul(buf[:nres], P, buf)
        torch.cuda.synchronize()
        bad = buf[:nres] != want
        assert not bad.any(), (form, int(bad.nonzero()[0]), int(bad.sum()))
        check_windows(lo, dev, P, n, nres, torch.float64, rng, shifts=(1, 4, 4097) if rep == 0 else (257,))


# ------------------------------------------------------------------------------------------------ kron
def kron_canary_one_launch(lo, dev):
    """Does the one-launch kron form run on this device (the XCD-map probe accepted it)? 512^2 f64, kron_fuse = 1."""
    rng = np.random.default_rng(0)
    A = torch.from_numpy(rng.uniform(-1, 1, (512, 512))).to(dev)
    K = lo.kron(A, A)
    x = torch.rand(512 * 512, dtype=torch.float64, device=dev)
    r = torch.empty_like(x)
    lo.mul(r, K, x)
    l0 = launches(lo)
    lo.mul(r, K, x)
    return launches(lo) - l0 == 1


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 3e-5)])
@pytest.mark.parametrize("m", [64, 512, 1024])
@pytest.mark.parametrize("fuse", [1, 0])
def test_kron_square(lo, dev, dtype, tol, m, fuse):
    ctx = lo.get_ctx(dev)
    one = kron_canary_one_launch(lo, dev)
    with ctx.tuned(kron_fuse=fuse):
        for rep in range(3):
            rng = np.random.default_rng(m + rep)
            A, B = rand(rng, m * m, dtype).reshape(m, m), rand(rng, m * m, dtype).reshape(m, m)
            col = lambda M: torch.from_numpy(np.ascontiguousarray(M.T)).to(dev).t()
            K = lo.kron(col(A), col(B))
            for op, tr in ((K, False), (K.T, True)):
                def want(v, ab, tr=tr):
                    a, b = ab_of(ab, dtype)
                    return oracle.kron_mul(v.astype(np.float64), A.astype(np.float64), B.astype(np.float64),
                                           v.astype(np.float64), a, b, trans=tr)
                check_aliased(lo, dev, op, rand(rng, m * m, dtype), dtype, want, tol)
            if m == 512 and fuse == 1 and one:
                # the separate-buffer call is the one-launch form, the aliased call leaves it for the two launches
                x = T(rand(rng, m * m, dtype), dev)
                r = torch.empty_like(x)
                l0 = launches(lo)
                lo.mul(r, K, x)
                assert launches(lo) - l0 == 1
                l0 = launches(lo)
                lo.mul(x, K, x)
                assert launches(lo) - l0 == 2


def test_kron_complex_and_diagonal(lo, dev):
    m = 64
    for rep in range(3):
        rng = np.random.default_rng(5 + rep)
        A = (rng.uniform(-1, 1, (m, m)) + 1j * rng.uniform(-1, 1, (m, m)))
        B = (rng.uniform(-1, 1, (m, m)) + 1j * rng.uniform(-1, 1, (m, m)))
        col = lambda M: torch.from_numpy(np.ascontiguousarray(M.T)).to(dev).t()
        K = lo.kron(col(A), col(B))
        Kd = np.kron(A, B)
        check_aliased(lo, dev, K, rand(rng, m * m, torch.complex128), torch.complex128,
                      lambda v, ab: ab_of(ab, None)[0] * (Kd @ v) + ab_of(ab, None)[1] * v, 1e-12)
        dA, dB = rng.uniform(-1, 1, 300), rng.uniform(-1, 1, 200)
        Kdd = lo.kron(lo.opDiagonal(T(dA, dev)), lo.opDiagonal(T(dB, dev)))
        dd = np.kron(dA, dB)
        check_aliased(lo, dev, Kdd, rng.uniform(-1, 1, 60_000), torch.float64,
                      lambda v, ab: ab_of(ab, None)[0] * (dd * v) + ab_of(ab, None)[1] * v, 1e-15)


# ------------------------------------------------------------------------------------------------ L-BFGS
def _pairs(rng, n, k):
    for _ in range(k):
        s = rng.uniform(-1, 1, n)
        yield s, s * rng.uniform(0.5, 2.0, n) + 1e-2 * rng.standard_normal(n)


LBFGS_CASES = [(1 << 12, 5, None), (1 << 12, 10, None), (1 << 20, 5, 1), (1 << 20, 10, 0), (1 << 24, 5, None)]


@pytest.mark.parametrize("n,mem,park", LBFGS_CASES)
@pytest.mark.parametrize("kind,mode", [("inv", "twopass"), ("inv", "reforder"), ("fwd", "gram"), ("fwd", "reforder"),
                                       ("fwd", "compact")])
def test_lbfgs(lo, dev, n, mem, park, kind, mode):
    ctx = lo.get_ctx(dev)
    # 2^20: the persistent apply, LDS parking on / off
    with ctx.tuned(**({"qn_persist_min_bytes": 0, "qn_persist_lds": park} if park is not None else {})):
        for rep in range(3 if n < (1 << 24) else 1):
            rng = np.random.default_rng(n + mem + rep)
            make = lo.InverseLBFGSOperator if kind == "inv" else lo.LBFGSOperator
            op = make(torch.float64, n, mem=mem, device=dev)
            if kind == "inv":
                op.set_mode(mode)
            else:
                op.set_push_mode(mode)
            ref = oracle.LBFGS(n, mem=mem, inverse=kind == "inv")
            for s, y in _pairs(rng, n, mem + 2):
                lo.push(op, T(s, dev), T(y, dev))
                ref.push(s, y)
            check_aliased(lo, dev, op, rng.uniform(-1, 1, n), torch.float64,
                          lambda v, ab: ref.mul(v.copy(), v, *ab_of(ab, None)), 1e-9)
            if kind == "inv" and rep == 0:
                check_windows(lo, dev, op, n, n, torch.float64, rng, shifts=SHIFTS if n < (1 << 24) else (4097,))


# ------------------------------------------------------------------------------------------------ wrappers, products
def test_products_and_wrappers(lo, dev):
    n = 3_000_001
    for rep in range(3):
        rng = np.random.default_rng(41 + rep)
        h = rng.uniform(-1, 1, n)
        h /= np.linalg.norm(h)
        d = rng.uniform(-1, 1, n)
        H, D = lo.opHouseholder(T(h, dev)), lo.opDiagonal(T(d, dev))

        def want(v, ab):
            a, b = ab_of(ab, None)
            return oracle.householder_mul(v.copy(), h, d * v, a, b)
        check_aliased(lo, dev, H * D, rng.uniform(-1, 1, n), torch.float64, want, 1e-12)
        check_aliased(lo, dev, lo.adjoint(H), rng.uniform(-1, 1, n), torch.float64,
                      lambda v, ab: oracle.householder_mul(v.copy(), h, v, *ab_of(ab, None)), 1e-12)


# ------------------------------------------------------------------------------------------------ graph capture
def test_aliased_call_inside_a_graph_capture(lo, dev):
    """The staging copy is a memcpy node of the captured graph: the replay reads the current x."""
    n = 1_000_000
    P = lo.opRestriction(lo.leaves.jrange(n, 1, -1), n, device=dev)
    x = torch.rand(n, dtype=torch.float64, device=dev)
    g = lo.graph.capture_mul(x, P, x)                      # warm-up (sizes the staging buffer), then the capture
    for rep in range(3):
        x_h = np.random.default_rng(rep).uniform(-1, 1, n)
        x.copy_(T(x_h, dev))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(x.cpu().numpy(), x_h[::-1])
