"""estimate_opnorm on the device: the two Krylov kernels of csrc/krylov.hip against numpy, and the restarted Lanczos of
linearoperators.jl_amd/opnorm.py end to end against dense numpy models (never the package's own to_dense).

Tolerance of the kernel comparisons. tests/tolerances.py has no class for fixed-order f64-accumulated dots, so the bound
is measured per shape: the rel-L2 distance between the numpy float64 evaluation and a numpy.longdouble evaluation of the
same inputs, times 8 (the kernel adds in another order than numpy; 8x covers the sqrt(n) spread of reorderings). For
Float32 data the inputs are rounded to float32 and the arithmetic is float64 — which is what the kernels do — and the
model additionally rounds w to float32 wherever the kernel STORES it (after each projection and after the division): a
Float32 vector cannot be closer to the exact result than its own rounding, so a bound without that term could be met by no
Float32 output at all. The reference the kernel is compared with stays the plain float64 evaluation."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import oracle
from tolerances import observe

gpu = pytest.mark.gpu
NP = {torch.float64: np.float64, torch.float32: np.float32}
NS = [1, 7, 255, 256, 257, 4099, 2 ** 20 + 3]
ORTH_SHAPES = [(n, k) for n in NS for k in (1, 2, 5, 20, 33) if k <= n]
COMBINE_SHAPES = [(n, k) for n in NS for k in (1, 5, 20) if k <= n]
DTYPES = [torch.float64, torch.float32]
NAMES = ("malloc", "free", "h2d", "d2h", "d2d", "d2h_bytes", "stream_sync", "device_sync", "event_sync", "memset_async",
         "launch", "blocking_copy")


def rel(a, b):
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (nb if nb else 1.0))


def inputs(n, k, npd, seed=0):
    rng = np.random.default_rng(1000 * k + n + seed)
    V = np.linalg.qr(rng.standard_normal((n, k)))[0]
    return np.asfortranarray(V.astype(npd)), rng.standard_normal(n).astype(npd), rng.standard_normal(k)


def cgs2(V, w, wt, store=lambda x: x, rounds=2):
    """Gram–Schmidt `rounds` times in the working type wt, w passing through `store` where the kernel stores it."""
    V, w = V.astype(wt), store(w.astype(wt))
    k = V.shape[1]
    coef = np.zeros(k + 1, wt)
    for _ in range(rounds):
        h = V.T @ w
        w = store(w - V @ h)
        coef[:k] += h
    beta = np.sqrt(w @ w)
    coef[k] = beta
    if beta > 0 and np.isfinite(beta):
        w = store(w / beta)
    return w, coef


def combine_ref(V, y, wt, store=lambda x: x):
    o = store(V.astype(wt) @ y.astype(wt))
    nrm = np.sqrt(o @ o)
    return (store(o / nrm) if nrm > 0 and np.isfinite(nrm) else o), nrm


def storage_rounding(npd):
    return (lambda x: x) if npd == np.float64 else (lambda x: x.astype(np.float32).astype(x.dtype))


class Basis:
    """k + 1 columns of leading dimension ldv on the device; column k is where a Lanczos loop keeps w."""

    def __init__(self, V, ldv, dtype, dev):
        n, k = V.shape
        host = np.zeros((k + 1, ldv), V.dtype)
        host[:k, :n] = V.T
        self.n, self.k, self.ldv = n, k, ldv
        self.t = torch.from_numpy(host.ravel()).to(dev)
        assert self.t.dtype == dtype

    def col(self, j):
        return self.t[j * self.ldv: j * self.ldv + self.n]

    def columns(self):
        return self.t.cpu().numpy().reshape(self.k + 1, self.ldv)[:self.k, :self.n].T


def off_phase(x, dev):
    """x on the device in storage that starts one element behind an aligned allocation: another 16-byte phase"""
    buf = torch.zeros(len(x) + 5, dtype=torch.from_numpy(x[:0]).dtype, device=dev)
    buf[1:len(x) + 1].copy_(torch.from_numpy(x))
    return buf, buf[1:len(x) + 1]


def ldvs(n, dtype):
    per16 = 16 // torch.empty(0, dtype=dtype).element_size()
    return [n, (n // per16 + 1) * per16]


def orth(lo, dev, basis, w, flags=0, ctx=None):
    ctx = ctx or lo.get_ctx(dev)
    coef = torch.full((basis.k + 1,), float("nan"), dtype=torch.float64, device=dev)
    st = lo._lib.lib().mxlo_krylov_orth(ctx.handle, lo._lib.F64 if basis.t.dtype == torch.float64 else lo._lib.F32,
                                        basis.t.data_ptr(), basis.ldv, basis.n, basis.k, w.data_ptr(), coef.data_ptr(), flags)
    return st, coef


def combine(lo, dev, basis, y_dev, out, ctx=None):
    ctx = ctx or lo.get_ctx(dev)
    coef = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    st = lo._lib.lib().mxlo_krylov_combine(ctx.handle, lo._lib.F64 if basis.t.dtype == torch.float64 else lo._lib.F32,
                                           basis.t.data_ptr(), basis.ldv, basis.n, basis.k, y_dev.data_ptr(), out.data_ptr(),
                                           coef.data_ptr())
    return st, coef


# ----------------------------------------------------------------------------------------------------- mxlo_krylov_orth
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,k", ORTH_SHAPES)
def test_orth_matches_numpy_cgs2(lo, dev, dtype, n, k):
    npd = NP[dtype]
    eps = float(np.finfo(npd).eps)
    V, w, _ = inputs(n, k, npd)
    w_ref, c_ref = cgs2(V, w, np.float64)
    w_ld, c_ld = cgs2(V, w, np.longdouble)
    w_mod, c_mod = cgs2(V, w, np.float64, storage_rounding(npd))
    tol_w, tol_c = 8 * rel(w_mod, w_ld), 8 * rel(c_mod, c_ld)
    for ldv in ldvs(n, dtype):
        for where in ("column k", "off phase"):
            basis = Basis(V, ldv, dtype, dev)
            if where == "column k":
                wt = basis.col(k)
                wt.copy_(torch.from_numpy(w))
            else:
                keep, wt = off_phase(w, dev)
            st, coef = orth(lo, dev, basis, wt)
            assert st == 0, lo._lib.lib().mxlo_last_error()
            w_out, c_out = wt.cpu().numpy().astype(np.float64), coef.cpu().numpy()
            e_w, e_c = rel(w_out, w_ref), rel(c_out, c_ref)
            print(f"orth n={n} k={k} {npd.__name__} ldv={ldv} {where}: w {e_w:.3e} (bound {tol_w:.3e}) coef {e_c:.3e} (bound {tol_c:.3e})")
            observe("krylov_orth w", e_w, dtype == torch.float32)
            observe("krylov_orth coef", e_c, dtype == torch.float32)
            assert np.array_equal(basis.columns(), V), "the basis columns are read-only"
            assert e_w <= tol_w and e_c <= tol_c, (ldv, where)
            V64 = V.astype(np.float64)
            assert np.abs(V64.T @ w_out).max() <= 4 * k * eps, (ldv, where)          # orthogonal after two rounds
            if k < n:                                   # k == n: w lies in span(V), a breakdown (tested below), not a unit vector
                assert abs(np.linalg.norm(w_out) - 1) <= 4 * eps * math.sqrt(n), (ldv, where)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,k", [(257, 5), (4099, 20), (2 ** 20 + 3, 2)])
def test_orth_breakdown(lo, dev, dtype, n, k):
    npd = NP[dtype]
    V, _, _ = inputs(n, k, npd)
    basis = Basis(V, ldvs(n, dtype)[1], dtype, dev)
    wt = basis.col(k)
    wt.copy_(torch.from_numpy(V[:, 0].copy()))                    # w in span(V) exactly
    st, coef = orth(lo, dev, basis, wt)
    c = coef.cpu().numpy()
    print(f"breakdown n={n} k={k} {npd.__name__}: beta {c[k]:.3e}")
    assert st == 0 and 0 <= c[k] <= 16 * float(np.finfo(npd).eps)
    assert abs(c[0] - 1) <= 8 * float(np.finfo(npd).eps)
    wt.zero_()                                                    # w = 0: beta == 0, nothing divided, no NaN
    st, coef = orth(lo, dev, basis, wt)
    c = coef.cpu().numpy()
    assert st == 0 and c[k] == 0 and np.array_equal(c, np.zeros(k + 1))
    assert np.array_equal(wt.cpu().numpy(), np.zeros(n, npd))


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_orth_dgks_is_decided_on_the_device(lo, dev, dtype):
    """MXLO_KRYLOV_DGKS: a w that is almost orthogonal to V already keeps |w| in the first round -> one round only (numpy
    with one round); a w dominated by its component in span(V) takes both rounds -> the bits of the unconditional call."""
    npd = NP[dtype]
    n, k = 4099, 5
    V, w, _ = inputs(n, k, npd)
    DGKS = lo._lib.KRYLOV_DGKS
    basis = Basis(V, ldvs(n, dtype)[1], dtype, dev)
    basis.col(k).copy_(torch.from_numpy(w))
    st, coef = orth(lo, dev, basis, basis.col(k), DGKS)
    w1, c1 = cgs2(V, w, np.float64, rounds=1)
    tol = 8 * rel(cgs2(V, w, np.float64, storage_rounding(npd), rounds=1)[1], cgs2(V, w, np.longdouble, rounds=1)[1])
    assert st == 0 and rel(coef.cpu().numpy(), c1) <= tol
    h2 = V.astype(np.float64).T @ cgs2(V, w, np.float64, rounds=1)[0]
    assert np.abs(h2).max() > 0 and not np.array_equal(coef.cpu().numpy(), cgs2(V, w, np.float64)[1])   # a second round would show
    w_in = (V[:, 0] + npd(1e-3) * w).astype(npd)
    outs = []
    for flags in (0, DGKS):
        basis.col(k).copy_(torch.from_numpy(w_in))
        st, coef = orth(lo, dev, basis, basis.col(k), flags)
        assert st == 0
        outs.append((basis.col(k).cpu().numpy(), coef.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


# -------------------------------------------------------------------------------------------------- mxlo_krylov_combine
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,k", COMBINE_SHAPES)
def test_combine_matches_numpy(lo, dev, dtype, n, k):
    npd = NP[dtype]
    V, _, y = inputs(n, k, npd)
    o_ref, nrm_ref = combine_ref(V, y, np.float64)
    o_ld, nrm_ld = combine_ref(V, y, np.longdouble)
    o_mod, nrm_mod = combine_ref(V, y, np.float64, storage_rounding(npd))
    tol_o, tol_n = 8 * rel(o_mod, o_ld), 8 * rel(nrm_mod, nrm_ld)
    y_dev = torch.from_numpy(y).to(dev)
    for ldv in ldvs(n, dtype):
        for where in ("column 0", "off phase"):
            basis = Basis(V, ldv, dtype, dev)
            if where == "column 0":
                out = basis.col(0)                                 # the restart vector overwrites the basis
            else:
                keep, out = off_phase(np.zeros(n, npd), dev)
            st, coef = combine(lo, dev, basis, y_dev, out)
            assert st == 0, lo._lib.lib().mxlo_last_error()
            e_o, e_n = rel(out.cpu().numpy(), o_ref), rel(coef.cpu().numpy()[0], nrm_ref)
            print(f"combine n={n} k={k} {npd.__name__} ldv={ldv} {where}: out {e_o:.3e} (bound {tol_o:.3e}) norm {e_n:.3e} (bound {tol_n:.3e})")
            observe("krylov_combine out", e_o, dtype == torch.float32)
            assert e_o <= tol_o and e_n <= tol_n, (ldv, where)
            first = 1 if where == "column 0" else 0                # every other column is untouched
            assert np.array_equal(basis.columns()[:, first:], V[:, first:])


@gpu
def test_combine_refuses_a_partial_overlap(lo, dev):
    V, _, y = inputs(257, 5, np.float64)
    basis = Basis(V, 258, torch.float64, dev)
    st, _ = combine(lo, dev, basis, torch.from_numpy(y).to(dev), basis.t[3:3 + 257])
    assert st == lo._lib.EINVAL
    st, _ = orth(lo, dev, basis, basis.col(4))                     # w inside the first k columns
    assert st == lo._lib.EINVAL


# ------------------------------------------------------------------------------------- reproducibility, runtime contract
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,k", [(4099, 20), (2 ** 20 + 3, 5)])
def test_orth_is_bit_reproducible(lo, dev, dtype, n, k):
    npd = NP[dtype]
    V, w, _ = inputs(n, k, npd)
    basis = Basis(V, ldvs(n, dtype)[1], dtype, dev)
    runs = []
    for _ in range(2):
        basis.col(k).copy_(torch.from_numpy(w))
        st, coef = orth(lo, dev, basis, basis.col(k))
        assert st == 0
        runs.append((basis.col(k).cpu().numpy(), coef.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def snap(lo):
    a = (C.c_int64 * 12)()
    lo._lib.call("mxlo_debug_counters", a)
    return dict(zip(NAMES, list(a)))


@gpu
def test_warmed_kernels_only_launch_and_a_cycle_copies_once(lo, dev):
    import gc
    n, k = 100_003, 10
    V, w, y = inputs(n, k, np.float64)
    basis = Basis(V, ldvs(n, torch.float64)[1], torch.float64, dev)
    basis.col(k).copy_(torch.from_numpy(w))
    y_dev = torch.from_numpy(y).to(dev)
    coef = torch.zeros(k + 1, dtype=torch.float64, device=dev)
    ctx, L = lo.get_ctx(dev), lo._lib.lib()
    calls = {
        "orth": lambda: L.mxlo_krylov_orth(ctx.handle, 0, basis.t.data_ptr(), basis.ldv, n, k, basis.col(k).data_ptr(), coef.data_ptr(), 1),
        "combine": lambda: L.mxlo_krylov_combine(ctx.handle, 0, basis.t.data_ptr(), basis.ldv, n, k, y_dev.data_ptr(), basis.col(0).data_ptr(), coef.data_ptr()),
    }
    for name, fn in calls.items():
        assert fn() == 0                                           # warm-up
        gc.collect()
        torch.cuda.synchronize()
        a = snap(lo)
        assert fn() == 0
        b = snap(lo)
        torch.cuda.synchronize()
        d = {key: b[key] - a[key] for key in NAMES}
        assert d["launch"] >= 1 and not {key: v for key, v in d.items() if key != "launch" and v}, (name, d)
    # one full Lanczos cycle of estimate_opnorm: exactly one device-to-host copy, nothing allocated, nothing else copied
    D = lo.opDiagonal(torch.linspace(-3, 2, 1023, dtype=torch.float64, device=dev))
    lo.estimate_opnorm(D, tol=1e-6)                                # warm
    lo.opnorm._last_cycle_counters = None
    lo.estimate_opnorm(D, tol=1e-6)
    d = dict(zip(NAMES, lo.opnorm._last_cycle_counters))
    assert d["d2h"] == 1 and d["stream_sync"] == 1 and d["launch"] > 0
    assert not {key: v for key, v in d.items() if key not in ("launch", "d2h", "d2h_bytes", "stream_sync") and v}, d


@gpu
def test_sharded_ctx_is_refused(lo, dev):
    """With an all-reduce hook installed both calls return MXLO_ESTATE and never call the hook."""
    V, w, y = inputs(257, 5, np.float64)
    basis = Basis(V, 258, torch.float64, dev)
    basis.col(5).copy_(torch.from_numpy(w))
    called = []
    ctx = lo.Context(dev.index)

    def hook(user, buf, count, stream):
        called.append(count)
        return 0

    ctx.set_allreduce(hook)
    try:
        st, _ = orth(lo, dev, basis, basis.col(5), ctx=ctx)
        assert st == lo._lib.ESTATE and b"all-reduce" in lo._lib.lib().mxlo_last_error()
        st, _ = combine(lo, dev, basis, torch.from_numpy(y).to(dev), basis.col(0), ctx=ctx)
        assert st == lo._lib.ESTATE
    finally:
        ctx.set_allreduce(None)
    torch.cuda.synchronize()
    assert not called and np.array_equal(basis.columns(), V)


# ------------------------------------------------------------------------------------------------------------ end to end
# Dense numpy models. `chosen` marks the spectra picked here, which must keep the top eigenvalue (singular value) at least
# 5 % of the answer away from the next one; the cases with a prescribed spectrum (the linspace diagonal, whose
# gap is 5 / 1022, opEye and opHouseholder, whose Krylov space is invariant after one or two steps, opZeros) are not.
def sym_with_gap(rng, n, top=4.0):
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    lam = rng.uniform(-1, 1, n)
    lam[0] = -top
    return (Q * lam) @ Q.T


def qn_pairs(rng, n, k, last):
    """k pairs with curvatures in [0.5, 2]; the last one scaled by `last`, which sets the top eigenvalue apart"""
    out = []
    for i in range(k):
        s = rng.uniform(-1, 1, n)
        out.append((s, s * rng.uniform(0.5, 2.0, n) * (last if i == k - 1 else 1.0) + 1e-2 * rng.standard_normal(n)))
    return out


def oracle_dense(O, n):
    M, e = np.zeros((n, n)), np.zeros(n)
    for i in range(n):
        e[i] = 1
        M[:, i] = O.mul(np.zeros(n), e, 1.0, 0.0)
        e[i] = 0
    return M


def model(name):
    """(data for the device operator, dense float64 model, the model is Hermitian)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "hermitian":
        A = sym_with_gap(rng, 300)
        return A, A, True
    if name in ("dense 257x129", "dense 129x257"):
        m, n = (257, 129) if name.endswith("129") else (129, 257)
        M = rng.standard_normal((m, n))
        u, v = rng.standard_normal(m), rng.standard_normal(n)
        M += 40.0 * np.outer(u / np.linalg.norm(u), v / np.linalg.norm(v))
        return M, M, False
    if name in ("lbfgs", "inverse lbfgs", "lsr1"):
        n, mem = 500, 5
        pr = qn_pairs(rng, n, 7, 1 / 6 if name.startswith("inverse") else 6.0)
        # L-SR1 without scaling: with it the scaled identity carries the top eigenvalue n - mem times (no gap to measure)
        O = oracle.LSR1(n, mem=mem, scaling=False) if name == "lsr1" else oracle.LBFGS(n, mem=mem, scaling=True, inverse=name.startswith("inverse"))
        for s, y in pr:
            O.push(s.copy(), y.copy())
        return pr, oracle_dense(O, n), True
    if name == "adjoint(A)*A + D":
        A = rng.standard_normal((150, 200))
        v = rng.standard_normal(200)
        A += 30.0 * np.outer(rng.standard_normal(150) / math.sqrt(150), v / np.linalg.norm(v))
        d = rng.uniform(0.5, 1.5, 200)
        return (A, d), A.T @ A + np.diag(d), True
    if name == "diagonal 6":
        d = np.array([0.3, -0.7, 1.1, -2.5, 0.9, 2.0])
        return d, np.diag(d), True
    raise KeyError(name)


CHOSEN = ["hermitian", "dense 257x129", "dense 129x257", "lbfgs", "inverse lbfgs", "lsr1", "adjoint(A)*A + D", "diagonal 6"]


def reference_norm(M, hermitian):
    return float(np.abs(np.linalg.eigvalsh(M)).max()) if hermitian else float(np.linalg.norm(M, 2))


@pytest.mark.parametrize("name", CHOSEN)
def test_models_have_a_five_percent_gap(name):
    _, M, hermitian = model(name)
    if hermitian:
        assert np.abs(M - M.T).max() <= 1e-9 * np.abs(M).max()
        s = np.sort(np.abs(np.linalg.eigvalsh((M + M.T) / 2)))[::-1]
    else:
        s = np.linalg.svd(M, compute_uv=False)
    assert s[0] - s[1] >= 0.05 * s[0], (name, s[:3])
    shifted = np.sort(np.abs(np.linalg.eigvalsh(model("lbfgs")[1] + 0.5 * np.eye(500))))[::-1]
    assert shifted[0] - shifted[1] >= 0.05 * shifted[0]


def device_operator(lo, dev, name, dtype):
    data, M, hermitian = model(name)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev)
    if name == "hermitian":
        A = T(data.T).t()                                          # column-major
        op = lo.opHermitian(T(np.diag(data).copy()), A)
    elif name.startswith("dense"):
        op = lo.LinearOperatorFromMatrix(T(data.T).t())
    elif name in ("lbfgs", "inverse lbfgs", "lsr1"):
        ctor = {"lbfgs": lo.LBFGSOperator, "inverse lbfgs": lo.InverseLBFGSOperator, "lsr1": lo.LSR1Operator}[name]
        op = ctor(dtype, 500, mem=5, scaling=name != "lsr1", device=dev)
        for s, y in data:
            lo.push(op, T(s), T(y))
    elif name == "adjoint(A)*A + D":
        A = lo.LinearOperatorFromMatrix(T(data[0].T).t())
        op = lo.adjoint(A) * A + lo.opDiagonal(T(data[1]))
    elif name == "diagonal 6":
        op = lo.opDiagonal(T(data))
    if dtype == torch.float32:                                      # the model of what the device holds: Float32-rounded data
        if name in ("hermitian", "diagonal 6") or name.startswith("dense"):
            M = M.astype(np.float32).astype(np.float64)
    return op, M, hermitian


def check(lo, op, ref, dtype, **kw):
    tol = 1e-6 if dtype == torch.float64 else 1e-3
    value, converged = lo.estimate_opnorm(op, tol=tol, generator=kw.pop("generator", None), **kw)
    print(f"estimate_opnorm: {value!r} (reference {ref!r}, converged {converged})")
    assert converged is True and isinstance(value, float)
    assert abs(value - ref) <= tol * ref
    return value


@gpu
@pytest.mark.parametrize("name", CHOSEN)
def test_estimate_opnorm_chosen_models_f64(lo, dev, name):
    op, M, hermitian = device_operator(lo, dev, name, torch.float64)
    check(lo, op, reference_norm(M, hermitian), torch.float64)
    if name == "lbfgs":
        check(lo, lo.ShiftedOperator(op, 0.5), reference_norm(M + 0.5 * np.eye(500), True), torch.float64)


@gpu
@pytest.mark.parametrize("name", ["dense 257x129", "dense 129x257", "lbfgs"])
def test_estimate_opnorm_chosen_models_f32(lo, dev, name):
    op, M, hermitian = device_operator(lo, dev, name, torch.float32)
    check(lo, op, reference_norm(M, hermitian), torch.float32)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_estimate_opnorm_linspace_diagonal_negative_dominant(lo, dev, dtype):
    d = np.linspace(-3, 2, 1023).astype(NP[dtype])
    check(lo, lo.opDiagonal(torch.from_numpy(d).to(dev)), float(np.abs(d.astype(np.float64)).max()), dtype)


@gpu
def test_estimate_opnorm_invariant_subspaces(lo, dev):
    """opHouseholder (eigenvalues +-1: breakdown after two steps), opEye (after one), opZeros ((0.0, True))."""
    rng = np.random.default_rng(5)
    h = rng.standard_normal(4099)
    H = lo.opHouseholder(torch.from_numpy(h / np.linalg.norm(h)).to(dev))
    check(lo, H, 1.0, torch.float64)
    assert lo.opnorm._last_cycle_counters is not None
    S = lo.Storage(torch.float64, dev)
    check(lo, lo.opEye(torch.float64, 100, S=S), 1.0, torch.float64)
    assert lo.estimate_opnorm(lo.opZeros(torch.float64, 64, 64, S=S)) == (0.0, True)
    assert lo.estimate_opnorm(lo.opZeros(torch.float64, 70, 64, S=S)) == (0.0, True)


@gpu
@pytest.mark.parametrize("n", [1, 3, 5])
def test_estimate_opnorm_tiny_operators_take_the_dense_path(lo, dev, n):
    rng = np.random.default_rng(n)
    d = rng.uniform(-1, 1, n)
    d[0] = -3.0
    lo.opnorm._last_cycle_counters = None
    value, converged = lo.estimate_opnorm(lo.opDiagonal(torch.from_numpy(d).to(dev)))
    assert converged is True and abs(value - 3.0) <= 1e-14
    M = rng.standard_normal((n, n + 4))
    value, converged = lo.estimate_opnorm(lo.LinearOperatorFromMatrix(torch.from_numpy(M.T.copy()).to(dev).t()))
    assert converged and abs(value - np.linalg.norm(M, 2)) <= 1e-12 * np.linalg.norm(M, 2)
    assert lo.opnorm._last_cycle_counters is None                   # no Lanczos cycle ran


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_estimate_opnorm_large_diagonal(lo, dev, dtype):
    """n = 2^20 + 3: the reductions of both kernels span many workgroups."""
    n = 2 ** 20 + 3
    d = np.linspace(-1.0, 1.5, n).astype(NP[dtype])
    d[12345] = -2.0
    check(lo, lo.opDiagonal(torch.from_numpy(d).to(dev)), 2.0, dtype)


@gpu
def test_estimate_opnorm_reports_non_convergence(lo, dev):
    d = 1.0 - np.arange(1000) * 1e-9
    D = lo.opDiagonal(torch.from_numpy(d).to(dev))
    value, converged = lo.estimate_opnorm(D, ncv=3, maxiter=6, max_attempts=1, tol=1e-14)
    assert math.isnan(value) and converged is False


@gpu
def test_estimate_opnorm_is_deterministic_under_a_seed(lo, dev):
    op, M, hermitian = device_operator(lo, dev, "hermitian", torch.float64)
    runs = []
    for _ in range(2):
        g = torch.Generator(device=dev)
        g.manual_seed(1234)
        runs.append(lo.estimate_opnorm(op, tol=1e-6, generator=g))
    assert runs[0] == runs[1] and runs[0][1] is True


@gpu
def test_estimate_opnorm_rejections(lo, dev):
    z = torch.ones(8, dtype=torch.complex128, device=dev)
    with pytest.raises(TypeError, match="complex"):
        lo.estimate_opnorm(lo.opDiagonal(z))
    S = lo.Storage(torch.float64, dev)

    def prod(res, v, alpha, beta):
        res.copy_(v[:20] * alpha)

    op = lo.LinearOperator(torch.float64, 20, 30, False, False, prod, None, None, S=S)
    with pytest.raises(lo.LinearOperatorException):               # raised by the adjoint wrapper, not caught
        lo.estimate_opnorm(op)
