"""-m gpu: kron(A, B) (src/kron.jl:10-49) — factors aliased in place (column- and row-major), operator factors that
change state (push!), shapes off the tile grid, and the per-factor transposition entry point of the C ABI."""
import os

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

NP = {torch.float64: np.float64, torch.float32: np.float32}


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def colmajor(a, dev):
    """device matrix with Julia's (column-major) layout"""
    return torch.from_numpy(np.ascontiguousarray(a.T)).to(dev).t()


def rel(a, b):
    nb = np.linalg.norm(b.astype(np.float64))
    return np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / (nb if nb else 1.0)


def test_kat_kron_and_hermitian(lo, dev, kat):
    (c,) = [c for c in kat if c["kind"] == "kron"]
    A, B, K = np.array(c["A"]), np.array(c["B"]), np.array(c["K"])
    nK = np.linalg.norm(K, 1)
    for Af, Bf in ((colmajor(A, dev), colmajor(B, dev)), (T(A, dev), T(B, dev)),
                   (lo.LinearOperatorFromMatrix(colmajor(A, dev)), T(B, dev))):
        Kop = lo.kron(Af, Bf)
        assert np.linalg.norm((Kop * T(np.array(c["x"]), dev)).cpu().numpy() - np.array(c["expect_apply"]), 1) <= 1e-12 * nK
        assert np.linalg.norm((Kop.T * T(np.array(c["xt"]), dev)).cpu().numpy() - np.array(c["expect_tapply"]), 1) <= 1e-12 * nK
        assert np.linalg.norm((Kop.H * T(np.array(c["xt"]), dev)).cpu().numpy() - np.array(c["expect_tapply"]), 1) <= 1e-12 * nK
        res = T(np.array(c["res0"]), dev)
        lo.mul(res, Kop, T(np.array(c["x"]), dev), c["alpha"], c["beta"])
        assert np.linalg.norm(res.cpu().numpy() - np.array(c["expect_mul5"]), 1) <= 1e-12 * nK
        assert np.linalg.norm(lo.Matrix(Kop).cpu().numpy() - K, 1) <= 1e-15 * nK * K.shape[1]
    (c,) = [c for c in kat if c["kind"] == "dense"]                   # test_linop.jl:587-595, the reference's own numbers
    for Md in (colmajor(np.array(c["A"]), dev), T(np.array(c["A"]), dev)):
        op = lo.LinearOperatorFromMatrix(Md)
        for o in (op, op.T, op.H):                                    # A is symmetric
            y = torch.zeros(2, dtype=torch.float64, device=dev)
            lo.mul(y, o, T(np.array(c["x"]), dev))
            assert np.array_equal(y.cpu().numpy(), np.array(c["expect_apply"]))
            res = T(np.array(c["res0"]), dev)
            lo.mul(res, o, T(np.array(c["x"]), dev), c["alpha"], c["beta"])
            assert np.array_equal(res.cpu().numpy(), np.array(c["expect_mul5"]))
    (c,) = [c for c in kat if c["kind"] == "hermitian"]
    Hm = lo.opHermitian(T(np.array(c["d"]), dev), colmajor(np.array(c["A"]), dev))
    for op in (Hm, Hm.T, Hm.H):                                       # C is real symmetric: all three agree
        got = (op * T(np.array(c["v"]), dev)).cpu().numpy()
        assert np.linalg.norm(got - np.array(c["expect_apply"])) <= 1e-13 * np.linalg.norm(c["expect_apply"])
    res = T(np.array(c["res0"]), dev)
    lo.mul(res, Hm, T(np.array(c["x"]), dev), c["alpha"], c["beta"])
    assert np.linalg.norm(res.cpu().numpy() - np.array(c["expect_mul5"])) <= 1e-13 * np.linalg.norm(c["expect_mul5"])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("shapes", [((64, 64), (64, 64)), ((70, 34), (66, 130)), ((100, 100), (100, 100)),
                                    ((250, 30), (12, 260)), ((2, 4), (4, 2)), ((130, 2), (2, 130)),
                                    ((33, 65), (129, 31))])
def test_kron_shapes_and_layouts(lo, dev, dtype, shapes):
    """N and T applies for every combination of column-major / row-major factors (all four run the DMA GEMM with a
    transposition flag, nothing is copied), sizes off the 32/64/128 tile grid and odd extents (fallback kernel)."""
    (m, n), (p, q) = shapes
    rng = np.random.default_rng(m + 7 * n + 49 * p + 343 * q)
    npd = NP[dtype]
    A, B = (rng.standard_normal((m, n)) / 4).astype(npd), (rng.standard_normal((p, q)) / 4).astype(npd)
    K = np.kron(A.astype(np.float64), B.astype(np.float64))
    x, xt = rng.standard_normal(n * q).astype(npd), rng.standard_normal(m * p).astype(npd)
    r0 = rng.standard_normal(m * p).astype(npd)
    tol = 1e-12 if dtype == torch.float64 else 3e-5
    n1 = np.linalg.norm(K, 1)
    for Af in (colmajor(A, dev), T(A, dev)):
        for Bf in (colmajor(B, dev), T(B, dev)):
            ptrs = (Af.data_ptr(), Bf.data_ptr())
            Kop = lo.kron(Af, Bf)
            assert np.linalg.norm((Kop * T(x, dev)).cpu().numpy() - K @ x, 1) <= tol * n1 * max(1, np.abs(x).max())
            assert rel((Kop.T * T(xt, dev)).cpu().numpy(), K.T @ xt) <= 10 * tol
            res = T(r0.copy(), dev)
            lo.mul(res, Kop, T(x, dev), 2.0, 3.0)
            want = oracle.kron_mul(r0.copy(), A, B, x, 2.0, 3.0, flags=oracle.scalar_flags(npd, 2.0, 3.0))
            assert rel(res.cpu().numpy(), want) <= 10 * tol
            res = T(np.full(m * p, np.nan, dtype=npd), dev)
            lo.mul(res, Kop, T(x, dev), 1.0, 0.0)                      # beta == 0 never reads res
            assert torch.isfinite(res).all()
            assert ptrs == (Af.data_ptr(), Bf.data_ptr())


def test_kron_aliases_caller_matrices(lo, dev):
    """The reference's closure keeps A and B themselves (src/kron.jl:10-22): an in-place update of either factor
    after construction is seen by the next apply, for column-major AND row-major (torch default) storage."""
    rng = np.random.default_rng(3)
    A, B = rng.standard_normal((40, 24)), rng.standard_normal((16, 56))
    x = rng.standard_normal(24 * 56)
    for Af, Bf in ((colmajor(A, dev), colmajor(B, dev)), (T(A, dev), T(B, dev))):
        Kop = lo.kron(Af, Bf)
        assert rel((Kop * T(x, dev)).cpu().numpy(), np.kron(A, B) @ x) <= 1e-13
        Af.mul_(2.0)
        Bf[3, 5] = 7.0
        A2, B2 = 2.0 * A, B.copy()
        B2[3, 5] = 7.0
        assert rel((Kop * T(x, dev)).cpu().numpy(), np.kron(A2, B2) @ x) <= 1e-13
        xt = rng.standard_normal(40 * 16)
        assert rel((Kop.T * T(xt, dev)).cpu().numpy(), np.kron(A2, B2).T @ xt) <= 1e-13
    # a lower-precision factor is promoted into a converted copy: refreshed when the source changes
    Af32 = T(A.astype(np.float32), dev)
    Kop = lo.kron(Af32, colmajor(B, dev))
    Af32.add_(1.0)
    want = np.kron((A.astype(np.float32) + np.float32(1)).astype(np.float64), B) @ x
    assert rel((Kop * T(x, dev)).cpu().numpy(), want) <= 1e-13


def test_kron_of_live_quasi_newton_operator(lo, dev):
    """kron(LBFGSOperator, I) must follow the operator through push! / reset!: the reference re-materialises
    `Matrix(B*X*transpose(A))` from the operators on every apply (src/kron.jl:14-22)."""
    rng = np.random.default_rng(8)
    n, p = 12, 5
    Bq = lo.LBFGSOperator(torch.float64, n, mem=4, device=dev)
    I = torch.eye(p, dtype=torch.float64, device=dev)
    Kop = lo.kron(Bq, I)
    x = rng.standard_normal(n * p)

    def dense():
        return lo.Matrix(Bq).cpu().numpy()

    assert rel((Kop * T(x, dev)).cpu().numpy(), np.kron(np.eye(n), np.eye(p)) @ x) <= 1e-14     # empty memory: identity
    for it in range(6):                                               # wraps the circular buffer
        s = rng.standard_normal(n)
        y = s * rng.uniform(0.5, 2.0, n) + 1e-2 * rng.standard_normal(n)
        lo.push(Bq, T(s, dev), T(y, dev))
        want = np.kron(dense(), np.eye(p)) @ x
        assert rel((Kop * T(x, dev)).cpu().numpy(), want) <= 1e-12, it
        assert rel((Kop.T * T(x, dev)).cpu().numpy(), want) <= 1e-12, it            # symmetric
    lo.reset(Bq)
    assert rel((Kop * T(x, dev)).cpu().numpy(), x) <= 1e-14
    # composite factor: the state token follows the leaves underneath
    d = T(rng.uniform(1, 2, n), dev)
    comp = Bq + lo.opDiagonal(d)
    Kc = lo.kron(I, comp)
    lo.push(Bq, T(rng.standard_normal(n), dev), T(rng.standard_normal(n) + 3, dev))
    d.mul_(3.0)
    want = np.kron(np.eye(p), dense() + np.diag(d.cpu().numpy())) @ x
    assert rel((Kc * T(x, dev)).cpu().numpy(), want) <= 1e-12
    # an operator built from opaque closures cannot be tracked: it is re-materialised on every apply
    scale = [1.0]
    f = lo.LinearOperator(torch.float64, n, n, True, True, lambda res, v, a, b: lo.mul(res, lo.opEye(torch.float64, n, S=lo.Storage(torch.float64, dev)), v, a * scale[0], b),
                          None, None, S=lo.Storage(torch.float64, dev))
    Kf = lo.kron(f, I)
    assert rel((Kf * T(x, dev)).cpu().numpy(), x) <= 1e-14
    scale[0] = 5.0
    assert rel((Kf * T(x, dev)).cpu().numpy(), 5 * x) <= 1e-14


def test_kron_mul_ex_all_transposition_flags(lo, dev):
    """mxlo_kron_mul_ex directly: kron(opA, opB) for the four (trans_a, trans_b) combinations, incl. a padded
    leading dimension."""
    from linearoperators_jl_amd import _lib
    from linearoperators_jl_amd.device import get_ctx, ptr
    rng = np.random.default_rng(12)
    ctx = get_ctx(dev)
    for (am, an), (bp, bq) in (((64, 96), (128, 32)), ((70, 34), (66, 130)), ((5, 3), (4, 7))):
        A, B = rng.standard_normal((am, an)), rng.standard_normal((bp, bq))
        lda, ldb = am + 2, bp + 4
        Ad = torch.zeros(an, lda, dtype=torch.float64, device=dev)
        Ad[:, :am] = T(A.T, dev)
        Bd = torch.zeros(bq, ldb, dtype=torch.float64, device=dev)
        Bd[:, :bp] = T(B.T, dev)
        for ta in (0, 1):
            for tb in (0, 1):
                oA, oB = (A.T if ta else A), (B.T if tb else B)
                K = np.kron(oA, oB)
                x = rng.standard_normal(K.shape[1])
                r0 = rng.standard_normal(K.shape[0])
                res = T(r0.copy(), dev)
                work = torch.empty(oA.shape[0] * oB.shape[1], dtype=torch.float64, device=dev)
                _lib.call("mxlo_kron_mul_ex", ctx.handle, _lib.F64, ptr(res), ptr(Ad), am, an, lda, ta, ptr(Bd), bp, bq,
                          ldb, tb, ptr(T(x, dev)), ptr(work), 2.0, 3.0, 0)
                assert rel(res.cpu().numpy(), 2.0 * (K @ x) + 3.0 * r0) <= 1e-12, (am, an, bp, bq, ta, tb)


def test_kron_1000_and_transpose_rates_are_not_a_cliff(lo, dev):
    """Shapes off the 64-grid (1000^2) and the T mode used to fall to a generic kernel (4x slower); they now run the
    same DMA kernel: within 25 % of the 1024^2 N-mode time (timing assertions are loose: box-to-box spread)."""
    from linearoperators_jl_amd.device import Timer, get_ctx
    g = torch.Generator(device=dev).manual_seed(1)
    tm = Timer(get_ctx(dev))

    def t_us(n, transpose):
        A = ((torch.rand(n, n, dtype=torch.float64, device=dev, generator=g) * 2 - 1) / 32).t()
        B = ((torch.rand(n, n, dtype=torch.float64, device=dev, generator=g) * 2 - 1) / 32).t()
        x = torch.rand(n * n, dtype=torch.float64, device=dev, generator=g)
        out = torch.empty_like(x)
        K = lo.kron(A, B)
        op = K.T if transpose else K
        for _ in range(5):
            lo.mul(out, op, x, 1.0, 0.0)
        best = 1e9
        for _ in range(3):
            tm.start()
            for _ in range(20):
                lo.mul(out, op, x, 1.0, 0.0)
            tm.stop()
            best = min(best, tm.elapsed_ms() * 1e3 / 20)
        return best

    base = t_us(1024, False)
    assert t_us(1000, False) <= 1.25 * base
    assert t_us(1024, True) <= 1.35 * base


# ------------------------------------------------------------------------------------------ complex factors
def _cxa(a):
    a = np.array(a, dtype=np.float64)
    return a[..., 0] + 1j * a[..., 1]


def test_kat_complex_kron(lo, dev, kat):
    """test/test_kron.jl:3-36 with the Float64 A x ComplexF64 B pairing: T1 = kron(LinearOperator(A), B), T2 = kron(A,
    LinearOperator(B)), T3 = kron of both operators; Matrix(T), T*x, transpose(T)*x, T'*x against Base.kron(A, B) with
    the reference's bound eps()*norm(K,1) / 1e-12*norm(K,1); 5-arg mul! with complex alpha, beta."""
    (c,) = [c for c in kat if c["kind"] == "ckron"]
    A = np.array(c["A"])
    B = _cxa(c["B"])
    K = _cxa(c["K"])
    normK = np.abs(K).sum(axis=0).max()
    x, xt, r0 = _cxa(c["x"]), _cxa(c["xt"]), _cxa(c["res0"])
    At, Bt = T(A.T.copy(), dev).t(), T(B.T.copy(), dev).t()
    for Tk in (lo.kron(lo.LinearOperatorFromMatrix(At), Bt), lo.kron(At, lo.LinearOperatorFromMatrix(Bt)),
               lo.kron(lo.LinearOperatorFromMatrix(At), lo.LinearOperatorFromMatrix(Bt)), lo.kron(T(A, dev), T(B, dev))):
        assert Tk.eltype == torch.complex128 and Tk.shape == K.shape
        assert np.abs(lo.Matrix(Tk).cpu().numpy() - K).sum(axis=0).max() <= 4 * np.finfo(float).eps * normK
        assert np.abs(lo.Matrix(Tk.H).cpu().numpy() - K.conj().T).sum(axis=0).max() <= 4 * np.finfo(float).eps * normK
        assert np.abs(lo.Matrix(Tk.T).cpu().numpy() - K.T).sum(axis=0).max() <= 4 * np.finfo(float).eps * normK
        assert np.abs((Tk * T(x, dev)).cpu().numpy() - _cxa(c["expect_apply"])).sum() <= 1e-12 * normK
        assert np.abs((Tk.T * T(xt, dev)).cpu().numpy() - _cxa(c["expect_tapply"])).sum() <= 1e-12 * normK
        assert np.abs((Tk.H * T(xt, dev)).cpu().numpy() - _cxa(c["expect_ctapply"])).sum() <= 1e-12 * normK
        res = T(r0.copy(), dev)
        lo.mul(res, Tk, T(x, dev), complex(*c["alpha"]), complex(*c["beta"]))
        assert np.abs(res.cpu().numpy() - _cxa(c["expect_mul5"])).sum() <= 1e-12 * normK


@pytest.mark.parametrize("dtype,tol", [(torch.complex128, 1e-12), (torch.complex64, 5e-5)])
@pytest.mark.parametrize("shapes", [((1, 1), (1, 1)), ((3, 5), (4, 2)), ((17, 33), (9, 20)), ((64, 64), (64, 64)),
                                    ((130, 70), (33, 129)), ((96, 64), (48, 80))])
@pytest.mark.parametrize("kinds", ["cc", "rc", "cr"])
def test_complex_kron_vs_oracle_and_dense(lo, dev, dtype, tol, shapes, kinds):
    """complex x complex, real x complex, complex x real factors; prod!/tprod!/ctprod!, complex and real scalars, beta = 0
    not reading res; against the oracle's reference-literal restatement and against np.kron."""
    npc = np.complex128 if dtype == torch.complex128 else np.complex64
    npr = np.float64 if dtype == torch.complex128 else np.float32
    (m, n), (p, q) = shapes
    rng = np.random.default_rng(m * 7 + n * 5 + p * 3 + q + len(kinds))
    mk = lambda sh, cplx: ((rng.standard_normal(sh) + 1j * rng.standard_normal(sh)).astype(npc) if cplx
                           else rng.standard_normal(sh).astype(npr))
    A, B = mk((m, n), kinds[0] == "c"), mk((p, q), kinds[1] == "c")
    Kd = np.kron(A.astype(np.complex128), B.astype(np.complex128))
    Kop = lo.kron(T(A, dev), T(B.T.copy(), dev).t())              # one row-major, one column-major factor
    assert Kop.eltype == dtype
    for mode, Kx, o in (("N", Kd, Kop), ("T", Kd.T, Kop.T), ("C", Kd.conj().T, Kop.H)):
        nin, nout = Kx.shape[1], Kx.shape[0]
        x = (rng.standard_normal(nin) + 1j * rng.standard_normal(nin)).astype(npc)
        for (a, b) in ((complex(1), complex(0)), (2.0, -3.0), (1.5 - 0.5j, 0.25 + 2j)):
            r0 = (rng.standard_normal(nout) + 1j * rng.standard_normal(nout)).astype(npc)
            if b == 0:
                r0[:] = np.nan + 1j * np.nan
            res = T(r0.copy(), dev)
            lo.mul(res, o, T(x, dev), a, b)
            base = np.zeros(nout, npc) if b == 0 else r0.copy()
            want = oracle.kron_mul(base, A, B, x, a, b, trans={"N": False, "T": "T", "C": "C"}[mode],
                                   flags=oracle.scalar_flags(npc, a, b))
            scale = np.linalg.norm(Kx, 1) * np.abs(x).max() * abs(a) + abs(b) * (0 if b == 0 else np.abs(r0).max()) + 1e-300
            assert np.abs(res.cpu().numpy().astype(np.complex128) - want.astype(np.complex128)).max() <= tol * scale, (mode, a, b)
            dense = a * (Kx @ x.astype(np.complex128)) + (0 if b == 0 else b * r0.astype(np.complex128))
            assert np.abs(res.cpu().numpy().astype(np.complex128) - dense).max() <= 4 * tol * scale, (mode, a, b)


def test_complex_kron_tracks_factor_updates(lo, dev):
    """a complex matrix factor is split into planes once and re-split when the caller updates it in place."""
    rng = np.random.default_rng(9)
    A = T(rng.standard_normal((6, 4)) + 1j * rng.standard_normal((6, 4)), dev)
    B = T(rng.standard_normal((3, 5)), dev)
    K = lo.kron(A, B)
    x = T(rng.standard_normal(20) + 1j * rng.standard_normal(20), dev)
    for _ in range(2):
        want = np.kron(A.cpu().numpy(), B.cpu().numpy()) @ x.cpu().numpy()
        assert np.abs((K * x).cpu().numpy() - want).max() <= 1e-12 * np.abs(want).max()
        A.mul_(1.5 - 0.5j)
        B.add_(0.25)
        lo.touched(A)
        lo.touched(B)


@pytest.mark.parametrize("dtype,tol", [(torch.complex128, 1e-12), (torch.complex64, 5e-5)])
@pytest.mark.parametrize("shapes", [((40, 30), (20, 50)), ((64, 64), (64, 64)), ((7, 130), (33, 5)), ((96, 80), (40, 72))])
def test_gauss_form_matches_four_gemm_form(lo, dev, dtype, tol, shapes):
    """`mxlo_kron_mul_c3` (3 real GEMMs per complex product: k1 = (a+b)c, k2 = a(d-c), k3 = b(c+d)) against
    `mxlo_kron_mul_c` (4 real GEMMs) on the same planes, every factor mode (plain / transposed / conjugate-transposed),
    complex x complex, real x complex and complex x real factors, complex alpha / beta, and against numpy's kron within
    the reference's criterion 1e-12 * ||K||_1 (test/test_kron.jl:35). The three-multiplication form is normwise, not
    componentwise, accurate — which is what that criterion measures."""
    import ctypes as C
    from linearoperators_jl_amd import _lib
    from linearoperators_jl_amd.device import dtype_code, get_ctx
    ctx = get_ctx(dev)
    R = torch.float64 if dtype == torch.complex128 else torch.float32
    npr = np.float64 if dtype == torch.complex128 else np.float32
    (am, an), (bp, bq) = shapes
    rng = np.random.default_rng(am * 3 + bq)
    col = lambda M: torch.from_numpy(np.asfortranarray(M).T.copy()).to(dev).t()       # column-major device matrix
    for kinds in ("cc", "rc", "cr"):
        Ar, Ai = rng.standard_normal((am, an)).astype(npr), rng.standard_normal((am, an)).astype(npr)
        Br, Bi = rng.standard_normal((bp, bq)).astype(npr), rng.standard_normal((bp, bq)).astype(npr)
        if kinds[0] == "r":
            Ai = None
        if kinds[1] == "r":
            Bi = None
        dAr, dBr = col(Ar), col(Br)
        dAi, dBi = (col(Ai) if Ai is not None else None), (col(Bi) if Bi is not None else None)
        A = Ar + (1j * Ai if Ai is not None else 0)
        B = Br + (1j * Bi if Bi is not None else 0)
        for mode in (0, 1, 3):
            opA = A if mode == 0 else (A.T if mode == 1 else A.conj().T)
            opB = B if mode == 0 else (B.T if mode == 1 else B.conj().T)
            K = np.kron(opA.astype(np.complex128), opB.astype(np.complex128))
            nin, nout = K.shape[1], K.shape[0]
            x = (rng.standard_normal(nin) + 1j * rng.standard_normal(nin))
            r0 = (rng.standard_normal(nout) + 1j * rng.standard_normal(nout))
            xd = torch.from_numpy(x).to(dtype).to(dev)
            need = max(int(_lib.lib().mxlo_kron_c3_work_size(am, an, mode, bp, bq, mode)),
                       2 * (nin + max(an * bp, am * bq, an * bq, am * bp) + nout) + 24)
            work = torch.empty(need + 64, dtype=R, device=dev)
            out = {}
            sgn = -1.0 if mode & 2 else 1.0
            sums = []
            for re_, im_, r_, c_ in ((dAr, dAi, am, an), (dBr, dBi, bp, bq)):     # cached factor-sum planes (mxlo_plane_sum)
                if im_ is None:
                    sums.append(None)
                    continue
                sp = torch.empty(c_, r_, dtype=R, device=dev).t()
                _lib.call("mxlo_plane_sum", ctx.handle, dtype_code(dtype, True), sp.data_ptr(), re_.data_ptr(), im_.data_ptr(), r_, c_, r_, sgn)
                want_s = (re_.double() + sgn * im_.double()).to(R)
                assert torch.equal(sp, want_s)
                sums.append(sp)
            P_ = lambda t: None if t is None else t.data_ptr()
            for name in ("c3 cached sums", "c3 sums per call", "c4"):
                res = torch.from_numpy(r0).to(dtype).to(dev)
                if name == "c4":
                    _lib.call("mxlo_kron_mul_c", ctx.handle, dtype_code(dtype, True), res.data_ptr(), dAr.data_ptr(), P_(dAi), am, an, am, mode,
                              dBr.data_ptr(), P_(dBi), bp, bq, bp, mode, xd.data_ptr(), work.data_ptr(), 1.5, -0.5, 0.25, 2.0, 0)
                else:
                    cached = name == "c3 cached sums"
                    _lib.call("mxlo_kron_mul_c3", ctx.handle, dtype_code(dtype, True), res.data_ptr(), dAr.data_ptr(), P_(dAi),
                              P_(sums[0]) if cached else None, am, an, am, mode, dBr.data_ptr(), P_(dBi), P_(sums[1]) if cached else None,
                              bp, bq, bp, mode, xd.data_ptr(), work.data_ptr(), 1.5, -0.5, 0.25, 2.0, 0)
                out[name] = res.cpu().numpy().astype(np.complex128)
            want = (1.5 - 0.5j) * (K @ xd.cpu().numpy().astype(np.complex128)) + (0.25 + 2j) * torch.from_numpy(r0).to(dtype).numpy().astype(np.complex128)
            scale = np.abs(K).sum(axis=0).max() * max(1.0, np.abs(x).max())
            for name, got in out.items():
                assert np.abs(got - want).max() <= 4 * tol * scale, (name, kinds, mode)
            assert np.abs(out["c3 cached sums"] - out["c4"]).max() <= 4 * tol * scale, (kinds, mode)
            assert np.array_equal(out["c3 cached sums"], out["c3 sums per call"]), (kinds, mode)     # same arithmetic


def test_complex_form_switch_and_what_each_form_guarantees(lo, dev):
    """`kron(A, B, complex_form=...)`: the Gauss form (default, 3 real GEMMs per complex product) is NORMWISE accurate,
    the 4-GEMM form COMPONENTWISE. Data whose imaginary parts are 1e-9 of the real parts separates the two: both meet
    the reference's normwise criterion (test/test_kron.jl:35, 1e-12 * ||K||_1), but only the 4-GEMM form keeps the tiny
    imaginary part of K*x to a relative 1e-10 — the Gauss form forms it as a difference of O(1) products and is allowed
    to lose it (its absolute error still sits at the eps * ||K|| * ||x|| level)."""
    rng = np.random.default_rng(4242)
    m, p = 48, 40
    tiny = 1e-9
    A = rng.uniform(0.5, 1.5, (m, m)) + 1j * tiny * rng.uniform(0.5, 1.5, (m, m))
    B = rng.uniform(0.5, 1.5, (p, p)) + 1j * tiny * rng.uniform(0.5, 1.5, (p, p))
    x = rng.uniform(0.5, 1.5, m * p) + 0j
    dA, dB = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    dx = torch.from_numpy(x).to(dev)
    # exact-enough reference: products of the planes in extended precision (every term positive: no cancellation)
    Al, Bl = A.astype(np.clongdouble), B.astype(np.clongdouble)
    X = x.astype(np.clongdouble).reshape(m, p).T              # q x n, column-major vec
    want = (Bl @ X @ Al.T).T.reshape(-1)
    K1 = np.abs(np.kron(A, B)).sum(axis=0).max()
    got = {}
    for form in ("gauss", "4gemm"):
        K = lo.kron(dA, dB, complex_form=form)
        assert K.complex_form == form
        got[form] = (K * dx).cpu().numpy()
        assert np.abs(got[form] - want).max() <= 1e-12 * K1 * np.abs(x).max(), form      # the reference's criterion
    rel_im = {f: float((np.abs(got[f].imag - want.imag) / np.abs(want.imag)).max()) for f in got}
    assert rel_im["4gemm"] <= 1e-10, rel_im
    # the Gauss form's imaginary part is only absolutely accurate: eps * |re| scale, i.e. ~1e-16 / 1e-9 relative
    assert float(np.abs(got["gauss"].imag - want.imag).max()) <= 64 * np.finfo(np.float64).eps * float(np.abs(want.real).max()) * m
    assert lo.kron(dA, dB).complex_form == ("gauss" if os.environ.get("MXLO_KRON_GAUSS", "1") != "0" else "4gemm")
    with pytest.raises(ValueError):
        lo.kron(dA, dB, complex_form="karatsuba")


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 3e-5)])
@pytest.mark.parametrize("shape", [((64, 64), (64, 64)), ((128, 96), (200, 160)), ((256, 256), (256, 256)), ((300, 260), (180, 340)),
                                   ((512, 512), (512, 512)), ((1024, 1024), (1024, 1024)), ((520, 1000), (1000, 520))])
def test_kron_one_launch_form_is_bit_identical_to_the_two_launches(lo, dev, dtype, tol, shape):
    """Round 6: where every tile of both GEMMs of a kron apply has its own CU, the two dependent products run as ONE launch
    whose dependency never leaves an XCD (gemm_glds.h: kron_fused_kernel; tune key kron_fuse). Same tiles, same MFMA order
    per tile: `mul!`, the 5-arg form and the transposed product have the BITS of the two-launch schedule, on and off the
    tile grid, repeatedly (the counters re-arm themselves), and the result is the dense Kronecker product's."""
    (am, an), (bp, bq) = shape
    npd = NP[dtype]
    rng = np.random.default_rng(am + 3 * an + 5 * bp + 7 * bq)
    A, B = rng.uniform(-1, 1, (am, an)).astype(npd), rng.uniform(-1, 1, (bp, bq)).astype(npd)
    K = lo.kron(colmajor(A, dev), colmajor(B, dev))
    x, xt = T(rng.uniform(-1, 1, an * bq).astype(npd), dev), T(rng.uniform(-1, 1, am * bp).astype(npd), dev)
    r0 = T(rng.uniform(-1, 1, am * bp).astype(npd), dev)
    ctx = lo.get_ctx(dev)
    got = {}
    for fuse in (0, 1):
        with ctx.tuned(kron_fuse=fuse):
            out = []
            for rep in range(3):                                  # repeated applies: the counters of the fused form re-arm themselves
                a = torch.full((am * bp,), float("nan"), dtype=dtype, device=dev)
                lo.mul(a, K, x)
                b = r0.clone()
                lo.mul(b, K, x, 0.75, -1.25)
                c = torch.full((an * bq,), float("nan"), dtype=dtype, device=dev)
                lo.mul(c, K.T, xt)
                out.append((a, b, c))
            torch.cuda.synchronize()
            for rep in (1, 2):
                assert all(torch.equal(u, v) for u, v in zip(out[0], out[rep]))
            got[fuse] = out[0]
    assert all(torch.equal(u, v) for u, v in zip(got[0], got[1]))
    if am * bp * an * bq <= 1 << 26:                               # the dense product as the reference's test does (test_kron.jl:35)
        Kd = np.kron(A.astype(np.float64), B.astype(np.float64))
        assert rel(got[1][0].cpu().numpy(), Kd @ x.cpu().numpy().astype(np.float64)) <= tol
        assert rel(got[1][2].cpu().numpy(), Kd.T @ xt.cpu().numpy().astype(np.float64)) <= tol


def test_one_launch_kron_timeout_is_an_error_not_a_hang(lo, dev):
    """The consumers of the one-launch kron wait for the producers of their row block. If one never signals (not co-resident,
    a dispatch that broke the XCD round-robin; here: the `fused_debug_drop` test hook), the wait must END — the affected tiles
    stored as NaN, ctx fault word raised —, the next call must say so, and the ctx stays usable on the two-launch schedule,
    its counters re-armed."""
    import time
    ctx = lo.get_ctx(dev)
    rng = np.random.default_rng(23)
    n = 256
    A, B = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    K = lo.kron(colmajor(A, dev), colmajor(B, dev))
    x = T(rng.uniform(-1, 1, n * n), dev)
    res = torch.zeros(n * n, dtype=torch.float64, device=dev)
    want = (B @ x.cpu().numpy().reshape(n, n, order="F") @ A.T).reshape(-1, order="F")
    # a fault switches all the single-launch forms off: the exit of this block puts them back
    with ctx.tuned(kron_fuse=1, house_fused=1, qn_fused_small=1, qn_persist=1, herm_single=1):
        lo.mul(res, K, x, 1.0, 0.0)
        torch.cuda.synchronize()
        assert rel(res.cpu().numpy(), want) <= 1e-12
        with ctx.tuned(fused_timeout_ms=30):
            with ctx.tuned(fused_debug_drop=3):
                t0 = time.perf_counter()
                lo.mul(res, K, x, 1.0, 0.0)          # the launch succeeds; the consumers of workgroup 3's row block give up
                torch.cuda.synchronize()
                assert time.perf_counter() - t0 < 5.0
                got = res.cpu().numpy()
                assert np.isnan(got).any() and not np.isnan(got).all(), "the tiles behind the missing producer are NaN, the others are not"
            with pytest.raises(Exception, match="timed out"):
                lo.mul(res, K, x, 1.0, 0.0)          # reported (and repaired) at the next apply
            lo.mul(res, K, x, 1.0, 0.0)              # the one-launch form is off now: two launches
            torch.cuda.synchronize()
            assert rel(res.cpu().numpy(), want) <= 1e-12
            with ctx.tuned(kron_fuse=1):             # counters were re-armed: the one launch works again, repeatedly
                for _ in range(4):
                    res.zero_()
                    lo.mul(res, K, x, 1.0, 0.0)
                torch.cuda.synchronize()
                assert rel(res.cpu().numpy(), want) <= 1e-12


# ---- the one-launch form: where it runs, and its edge shapes ------------------------------------------------------------
def _launches(lo):
    import ctypes as C
    a = (C.c_int64 * 12)()
    lo._lib.call("mxlo_debug_counters", a)
    return a[10]


def _kron_launches(lo, res, K, x, *ab):
    """kernel launches of one (warmed) apply"""
    lo.mul(res, K, x, *ab)
    l0 = _launches(lo)
    lo.mul(res, K, x, *ab)
    return _launches(lo) - l0


def _one_launch_canary(lo, dev):
    """512^2 f64 with kron_fuse = 1: True when the one-time XCD-map probe (dense.hip: xcd_map_ok) accepted this device."""
    rng = np.random.default_rng(1)
    K = lo.kron(colmajor(rng.uniform(-1, 1, (512, 512)), dev), colmajor(rng.uniform(-1, 1, (512, 512)), dev))
    x = T(rng.uniform(-1, 1, 512 * 512), dev)
    return _kron_launches(lo, torch.empty_like(x), K, x) == 1


def _fused_gate(shape, dtype, num_cu):
    """kron_t's one-launch gate (dense.hip) restated for kron(A, B) * x with column-major A (m x n), B (p x q), no
    transposition, 16-byte aligned device buffers: the DMA preconditions of both GEMMs, one tile class below 128 for
    both products (tile_of), every tile on its own CU (grid <= num_cu), at most 64 row blocks."""
    (m, n), (p, q) = shape
    vec = 16 // (8 if dtype == torch.float64 else 4)
    if min(m, q, p) < vec or m % vec or q % vec or p % vec:
        return False

    def tile_of(M, N):
        tiles = lambda t: -(-M // t) * -(-N // t)
        if tiles(128) >= num_cu:
            return 128
        return 64 if tiles(64) * 5 >= num_cu * 3 else 32
    t1, t2 = tile_of(m, q), tile_of(p, m)
    if t1 != t2 or t1 == 128:
        return False
    nrb, gy1, gx2 = -(-m // t1), -(-q // t1), -(-p // t1)
    grid = 8 * (-(-nrb // 8) * max(gy1, gx2))
    return grid <= num_cu and nrb <= 64


GATE_SHAPES = [((64, 64), (64, 64)), ((128, 96), (200, 160)), ((256, 256), (256, 256)), ((300, 260), (180, 340)),
               ((512, 512), (512, 512)), ((1024, 1024), (1024, 1024)), ((520, 1000), (1000, 520)),
               ((264, 512), (512, 512)), ((20, 512), (512, 512))]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_kron_one_launch_form_runs_wherever_the_gate_admits_it(lo, dev, dtype):
    """The bit-identity test above compares kron_fuse 0 with 1 and would pass with nothing checked if the one-launch form
    never ran. Here the launches are counted: one wherever the gate admits the shape, two with kron_fuse = 0 and two for
    an aliased call (res == x), which must leave the one-launch form."""
    if not _one_launch_canary(lo, dev):
        pytest.skip("the XCD-map probe (dense.hip: xcd_map_ok) rejected this device: kron never runs as one launch here")
    ctx = lo.get_ctx(dev)
    num_cu = ctx.info()["num_cu"]
    npd = NP[dtype]
    admitted = 0
    for shape in GATE_SHAPES:
        (am, an), (bp, bq) = shape
        rng = np.random.default_rng(am * bq)
        K = lo.kron(colmajor(rng.uniform(-1, 1, (am, an)).astype(npd), dev), colmajor(rng.uniform(-1, 1, (bp, bq)).astype(npd), dev))
        x = T(rng.uniform(-1, 1, an * bq).astype(npd), dev)
        res = torch.empty(am * bp, dtype=dtype, device=dev)
        gate = _fused_gate(shape, dtype, num_cu)
        admitted += gate
        with ctx.tuned(kron_fuse=1):
            got = _kron_launches(lo, res, K, x)
            assert got == 1 if gate else got >= 2, (shape, gate, got)
            if gate:
                assert _kron_launches(lo, res, K, x, 0.75, -1.25) == 1, shape
                with ctx.tuned(kron_fuse=0):
                    assert _kron_launches(lo, res, K, x) == 2, shape
                if am * bp == an * bq:                                # square: mul!(x, K, x)
                    l0 = _launches(lo)
                    lo.mul(x, K, x)
                    assert _launches(lo) - l0 == 2, shape
    assert admitted >= 4


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 3e-5)])
@pytest.mark.parametrize("shape", [((264, 512), (512, 512)), ((20, 512), (512, 512)), ((20, 64), (64, 20))])
def test_kron_one_launch_form_on_row_blocks_that_share_a_cache_line(lo, dev, dtype, tol, shape):
    """m * sizeof(T) % 128 != 0: a 128-byte line of Ut straddles two row blocks — with nrb = 9 (== 1 mod 8) the last row
    block of one column and block 0 of the next sit on the same XCD — and m = 20, a single row block. Every element is
    checked against the oracle and against the two-launch bits, with fresh x three times."""
    (am, an), (bp, bq) = shape
    npd = NP[dtype]
    ctx = lo.get_ctx(dev)
    rng = np.random.default_rng(am + bp)
    A, B = rng.uniform(-1, 1, (am, an)).astype(npd), rng.uniform(-1, 1, (bp, bq)).astype(npd)
    K = lo.kron(colmajor(A, dev), colmajor(B, dev))
    for rep in range(3):
        xh = rng.uniform(-1, 1, an * bq).astype(npd)
        x = T(xh, dev)
        got = {}
        for fuse in (1, 0):
            with ctx.tuned(kron_fuse=fuse):
                got[fuse] = torch.full((am * bp,), float("nan"), dtype=dtype, device=dev)
                lo.mul(got[fuse], K, x)
        assert torch.equal(got[1], got[0]), (rep, int((got[1] != got[0]).nonzero()[0]))
        want = oracle.kron_mul(np.empty(am * bp), A.astype(np.float64), B.astype(np.float64), xh.astype(np.float64), 1.0, 0.0)
        err = np.abs(got[1].cpu().numpy().astype(np.float64) - want) / (np.abs(want) + np.abs(want).max() * 1e-3)
        assert err.max() <= tol * 100, (rep, int(err.argmax()), float(err.max()))
        assert rel(got[1].cpu().numpy(), want) <= tol


def test_kron_after_the_no_wait_mode_matches_the_oracle(lo, dev):
    """kron_fuse = 2 (timing experiment, documented wrong results) can leave the row-block counters non-zero; setting
    kron_fuse back to 1 re-arms them, so the next apply is right again."""
    ctx = lo.get_ctx(dev)
    rng = np.random.default_rng(3)
    A, B = rng.uniform(-1, 1, (512, 512)), rng.uniform(-1, 1, (512, 512))
    K = lo.kron(colmajor(A, dev), colmajor(B, dev))
    xh = rng.uniform(-1, 1, 512 * 512)
    x, res = T(xh, dev), torch.empty(512 * 512, dtype=torch.float64, device=dev)
    want = oracle.kron_mul(np.empty(512 * 512), A, B, xh, 1.0, 0.0)
    with ctx.tuned(kron_fuse=2):
        for _ in range(3):
            lo.mul(res, K, x)
        torch.cuda.synchronize()
    for _ in range(3):
        res.fill_(float("nan"))
        lo.mul(res, K, x)
        assert rel(res.cpu().numpy(), want) <= 1e-12
