"""opLDL of a dense symmetric matrix on the device (csrc/linalg.hip, linearoperators.jl_amd/linalg.py) against numpy in
Float64 on the host. The oracle has no solve.

Matrices. H = G G' + I with G = randn(n, n) / sqrt(n) from default_rng(5200 + n), symmetrised; signs s_i = -1 where
i % 3 == 2, else +1; K[i, j] = -H[i, j] where s_i = s_j = -1, else H[i, j]; K is rounded to the device precision. This is a
symmetric permutation of a quasi-definite [A B'; B -C] with A, C positive definite, so the unpivoted L D L' exists, with
negative pivots inside every block of NB = 64 and across block boundaries. Condition number 3.9 - 5.3, smallest |d| >= 1.3.

Sizes: those of test_gpu_linalg.py — 1, 5, NB - 1, NB, NB + 1, 2 NB + 1, 77 in a leading dimension of 79 with NaN in the
padding, and 2049 (33 block columns, the last one a single column).

Backward error bound. eta = |K x - v|_2 / (|K|_2 |x|_2) <= n eps(T) rho with rho = | |L||D||L'| |_2 / |K|_2: the normwise
form of the bound for a solve by a factorisation without pivoting, |dA| <= gamma_3n |L^||D^||L^'| (Higham, Accuracy and
Stability of Numerical Algorithms, Thm 11.3 with the substitutions of Thm 8.5), constants dropped as test_gpu_linalg.py drops
them. It is derived, not measured. L and D come from a blocked Float64 factorisation on the host (host_ldl below); rho is
between 1 (n = 1) and 61 (n = 2049). K is the matrix the device sees, x the device's result, both taken to Float64."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
NB = 64
NS = [1, 5, NB - 1, NB, NB + 1, 2 * NB + 1, 77, 2049]
LD = {77: 79}
DTYPES = [torch.float64, torch.float32]
NP = {torch.float64: np.float64, torch.float32: np.float32}
NAMES = ("malloc", "free", "h2d", "d2h", "d2d", "d2h_bytes", "stream_sync", "device_sync", "event_sync", "memset_async",
         "launch", "blocking_copy")


def host_ldl(K, nb=32):
    """Unpivoted K = L D L' in Float64: (unit lower L, d). Right-looking and blocked, so that the n^3 / 3 work is numpy
    matrix products; only the nb x nb diagonal blocks are eliminated column by column."""
    A = np.array(K, dtype=np.float64)
    n = A.shape[0]
    L, d = np.eye(n), np.zeros(n)
    for j0 in range(0, n, nb):
        j1 = min(n, j0 + nb)
        B = A[j0:j1, j0:j1].copy()
        Lk = np.eye(j1 - j0)
        for p in range(j1 - j0):
            d[j0 + p] = B[p, p]
            Lk[p + 1:, p] = B[p + 1:, p] / B[p, p]
            B[p + 1:, p + 1:] -= np.outer(Lk[p + 1:, p], B[p + 1:, p])
        L[j0:j1, j0:j1] = Lk
        if j1 < n:
            P = np.linalg.solve(Lk, A[j1:, j0:j1].T).T          # P = A_panel Lk^{-T} = L_panel D_k
            L[j1:, j0:j1] = P / d[j0:j1]
            A[j1:, j1:] -= L[j1:, j0:j1] @ P.T
    return L, d


def sym_norm2(S):
    return float(np.abs(np.linalg.eigvalsh(S)).max())


def facts(K):
    """(|K|_2, cond_2(K), negative eigenvalues, L, d, rho) of a symmetric K"""
    w = np.linalg.eigvalsh(K)
    nK = float(np.abs(w).max())
    L, d = host_ldl(K)
    rho = sym_norm2((np.abs(L) * np.abs(d)) @ np.abs(L).T) / nK
    return nK, nK / float(np.abs(w).min()), int((w < 0).sum()), L, d, rho


def seeded(n, npd):
    rng = np.random.default_rng(5200 + n)
    G = rng.standard_normal((n, n)) / np.sqrt(n)
    H = G @ G.T + np.eye(n)
    H = (H + H.T) / 2
    s = np.where(np.arange(n) % 3 == 2, -1.0, 1.0)
    K = np.where((s[:, None] < 0) & (s[None, :] < 0), -H, H)
    return K.astype(npd).astype(np.float64), H.astype(npd).astype(np.float64), rng.standard_normal(n).astype(npd).astype(np.float64)


@functools.lru_cache(maxsize=None)
def problem(n, npd):
    """(K, v, |K|_2, cond, number of negative eigenvalues, d, rho) in the precision the device gets, as Float64; computed
    once per (n, dtype), read-only."""
    K, _, v = seeded(n, npd)
    nK, cond, neg, _, d, rho = facts(K)
    for a in (K, v, d):
        a.setflags(write=False)
    return K, v, nK, cond, neg, d, rho


def dev_matrix(A, dtype, dev, ld=None, rowmajor=False):
    """A on the device: column-major in a leading dimension ld >= n (the padding holds NaN), or row-major."""
    n = A.shape[0]
    t = torch.from_numpy(np.ascontiguousarray(A)).to(dtype).to(dev)
    if rowmajor:
        return t.contiguous()
    ld = ld or max(n, 1)
    buf = torch.full((ld * A.shape[1],), float("nan"), dtype=dtype, device=dev)
    out = buf.as_strided(A.shape, (1, ld))
    out.copy_(t)
    return out


def dev_vec(x, dtype, dev):
    return torch.from_numpy(np.asarray(x)).to(dtype).to(dev)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def eta(A, norm2, x, v):
    nx = np.linalg.norm(x)
    return float(np.linalg.norm(A @ x - v) / (norm2 * nx)) if nx else float(np.linalg.norm(v))


def check_eta(tag, K, nK, rho, x, v, n, eps):
    assert np.isfinite(x).all(), tag
    e = eta(K, nK, x, v)
    print(f"eta {tag}: {e:.3e} = {e / (n * eps):.3e} n eps = {e / (n * eps * rho):.3e} n eps rho (rho = {rho:.2f})")
    # n eps(T) rho: derived (module docstring). Observed maxima on an MI355X: see DESIGN.md §4
    assert e <= n * eps * rho, (tag, e / (n * eps * rho))


# ------------------------------------------------------------------------------------------------ 1. backward error
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", NS)
def test_backward_error_of_the_solve_and_of_its_transpose_and_adjoint(lo, dev, n, dtype):
    K, v, nK, _, _, _, rho = problem(n, NP[dtype])
    op = lo.opLDL(dev_matrix(K, dtype, dev, LD.get(n)))
    vd = dev_vec(v, dtype, dev)
    eps = float(torch.finfo(dtype).eps)
    for name, w in (("op", op), ("transpose", lo.transpose(op)), ("adjoint", lo.adjoint(op))):
        res = torch.full((n,), float("nan"), dtype=dtype, device=dev)
        lo.mul(res, w, vd)
        check_eta(f"{name} n={n} {dtype}", K, nK, rho, host(res), v, n, eps)


# ------------------------------------------------------------------------------------------------ 2. the reference's own test
def simple_matrix(rng, n):
    """test/test_aux.jl:3-17 for a real element type: U S V' with singular values 1 .. 2"""
    U = np.linalg.qr(rng.random((n, n)))[0]
    V = np.linalg.qr(rng.random((n, n)))[0]
    return U @ np.diag(1 + np.arange(n) / (n - 1)) @ V.T


@gpu
def test_reference_test_cholesky_throws_and_ldl_solves_the_quasi_definite_matrix(lo, dev):
    """test/test_linop.jl:491-508: K = [A B'; B -C] is symmetric quasi-definite; opCholesky(K) throws PosDefException,
    |opLDL(K) (K e) - e| < sqrt(eps) |e| with e = ones, without and with check."""
    rng = np.random.default_rng(6)
    U = np.linalg.qr(rng.random((3, 3)))[0]
    A = U @ np.diag([1.0, 1.5, 2.0]) @ U.T
    B = simple_matrix(rng, 3)[:2]
    Q = np.linalg.qr(rng.random((2, 2)))[0]
    Cm = Q @ np.diag([1.0, 2.0]) @ Q.T
    K = np.block([[A, B.T], [B, -Cm]])
    K = (K + K.T) / 2
    Kd = dev_matrix(K, torch.float64, dev)
    with pytest.raises(lo.PosDefException):
        lo.opCholesky(Kd)
    e = np.ones(5)
    Ke = dev_vec(K @ e, torch.float64, dev)
    for check in (False, True):
        x = host(lo.apply(lo.opLDL(Kd, check=check), Ke))
        assert np.linalg.norm(x - e) < np.sqrt(np.finfo(np.float64).eps) * np.linalg.norm(e)


# ------------------------------------------------------------------------------------------------ 3. inertia
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [5, NB + 1, 2 * NB + 1])
def test_the_signs_of_d_are_the_inertia_and_d_is_the_hosts(lo, dev, n, dtype):
    """Sylvester's law of inertia: the negative pivots are as many as the negative eigenvalues. The pivots are the ratios
    of consecutive leading minors; a backward error n eps |K| moves them by cond(K) n eps relative (first order), normwise."""
    K, _, _, cond, neg, d, _ = problem(n, NP[dtype])
    op = lo.opLDL(dev_matrix(K, dtype, dev))
    assert op._d.dtype is torch.float64 and op._d.shape == (n,) and op._d.is_cuda
    got = host(op._d)
    assert int((got < 0).sum()) == neg == int((d < 0).sum())
    eps = float(torch.finfo(dtype).eps)
    rel = np.linalg.norm(got - d) / np.linalg.norm(d)
    print(f"d n={n} {dtype}: |d - d_host| / |d_host| = {rel:.3e} = {rel / (cond * n * eps):.3e} cond n eps")
    assert rel <= cond * n * eps


# ------------------------------------------------------------------------------------------------ 4. layouts, structure
@gpu
def test_row_major_matrices_are_read_in_place(lo, dev):
    n, dtype = 2 * NB + 1, torch.float64
    K, v, nK, _, _, _, rho = problem(n, np.float64)
    Kl = K.copy()
    Kl[np.tril_indices(n, -1)] = np.nan                     # only the upper triangle of the row-major M may be read
    Kd = dev_matrix(Kl, dtype, dev, rowmajor=True)
    assert Kd.stride(1) == 1
    op = lo.opLDL(Kd)
    vd = dev_vec(v, dtype, dev)
    for name, w in (("op", op), ("transpose", lo.transpose(op))):
        check_eta(f"row-major {name} n={n}", K, nK, rho, host(lo.apply(w, vd)), v, n, np.finfo(np.float64).eps)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_ldl_leaves_m_alone_reads_one_triangle_and_has_the_reference_flags(lo, dev, dtype):
    n = NB + 1
    K, v = problem(n, NP[dtype])[:2]
    Kd = dev_matrix(K, dtype, dev, n + 2)
    before = Kd.clone()
    op = lo.opLDL(Kd)
    assert torch.equal(Kd, before)
    assert op.symmetric and op.hermitian and lo.has_args5(op) and op.size() == (n, n) and op.eltype is dtype
    vd = dev_vec(v, dtype, dev)
    x = lo.apply(op, vd)
    Kn = K.copy()
    Kn[np.tril_indices(n, -1)] = np.nan                     # Symmetric(M, :U): the strict lower triangle is not read
    x2 = lo.apply(lo.opLDL(dev_matrix(Kn, dtype, dev, n + 2)), vd)
    assert torch.equal(x, x2)
    assert lo.nprod(op) == 1 and lo.ntprod(op) == 0
    lo.apply(lo.transpose(op), vd)                          # symmetric: transpose goes to prod!
    assert lo.nprod(op) == 2 and lo.ntprod(op) == 0


# ------------------------------------------------------------------------------------------------ 5. refusals
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_zero_pivot_in_a_later_block_column_raises_with_its_index(lo, dev, dtype):
    """blockdiag(K70, [0 1; 1 0], I57): the blocks are decoupled, every update of entry (71, 71) subtracts exact zeros, so
    pivot 71 (1-based, block column 2) is an exact zero."""
    n = 2 * NB + 1
    M = np.eye(n)
    M[:70, :70] = problem(70, NP[dtype])[0]
    M[70:72, 70:72] = [[0.0, 1.0], [1.0, 0.0]]
    with pytest.raises(lo.ZeroPivotException) as e:
        lo.opLDL(dev_matrix(M, dtype, dev))
    assert e.value.info == 71


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_zero_first_pivot_and_nan_pivot_raise_with_their_index(lo, dev, dtype):
    n = 2 * NB + 1
    K = problem(n, NP[dtype])[0].copy()
    K[0, 0] = 0.0
    with pytest.raises(lo.ZeroPivotException) as e:
        lo.opLDL(dev_matrix(K, dtype, dev))
    assert e.value.info == 1
    K = problem(n, NP[dtype])[0].copy()
    K[70, 70] = np.nan                                      # a pivot that is not finite
    with pytest.raises(lo.ZeroPivotException) as e:
        lo.opLDL(dev_matrix(K, dtype, dev))
    assert e.value.info == 71


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_check_true_refuses_non_symmetric_and_accepts_negative_definite(lo, dev, dtype):
    rng = np.random.default_rng(5)
    A = simple_matrix(rng, 5)
    with pytest.raises(lo.LinearOperatorException, match="not Hermitian"):
        lo.opLDL(dev_matrix(A, dtype, dev), check=True)
    n = NB + 1                                              # -H: no definiteness check, every pivot negative
    _, H, v = seeded(n, NP[dtype])
    nK, _, neg, _, _, rho = facts(-H)
    assert neg == n
    op = lo.opLDL(dev_matrix(-H, dtype, dev), check=True)
    assert int((host(op._d) < 0).sum()) == n
    x = host(lo.apply(op, dev_vec(v, dtype, dev)))
    check_eta(f"negative definite n={n} {dtype}", -H, nK, rho, x, v, n, float(torch.finfo(dtype).eps))


# ------------------------------------------------------------------------------------------------ 6. alpha and beta
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_alpha_beta_nan_in_res_and_res_is_v(lo, dev, dtype):
    """Against alpha * x_numpy + beta * res0. Tolerance: the forward error of a solve with backward error n eps rho is at
    most cond(K) n eps rho |x| (first order), the epilogue adds one rounding of each term:
    |got - want| <= (cond(K) n eps rho + 2 eps) (|alpha| |x| + |beta| |res0|)."""
    n = 2 * NB + 1
    K, v, _, cond, _, _, rho = problem(n, NP[dtype])
    op = lo.opLDL(dev_matrix(K, dtype, dev))
    eps = float(torch.finfo(dtype).eps)
    x = np.linalg.solve(K, v)
    rel = cond * n * eps * rho + 2 * eps
    rng = np.random.default_rng(3)
    res0 = rng.standard_normal(n).astype(NP[dtype]).astype(np.float64)
    vd = dev_vec(v, dtype, dev)
    for a, b in ((1.0, 0.0), (2.5, 0.0), (1.0, -0.5), (0.0, 3.0)):
        res = dev_vec(res0, dtype, dev)
        lo.mul(res, op, vd, a, b)
        tol = rel * (abs(a) * np.linalg.norm(x) + abs(b) * np.linalg.norm(res0))
        assert np.linalg.norm(host(res) - (a * x + b * res0)) <= tol, (a, b)
        if b == 0:                                          # beta == 0: res is not read
            res = torch.full((n,), float("nan"), dtype=dtype, device=dev)
            lo.mul(res, op, vd, a, b)
            assert np.isfinite(host(res)).all()
            assert np.linalg.norm(host(res) - a * x) <= rel * abs(a) * np.linalg.norm(x)
        xv = vd.clone()                                     # res is v: alpha K^{-1} v + beta v
        lo.mul(xv, op, xv, a, b)
        tol = rel * (abs(a) * np.linalg.norm(x) + abs(b) * np.linalg.norm(v))
        assert np.linalg.norm(host(xv) - (a * x + b * v)) <= tol, (a, b)


@gpu
def test_partial_overlap_of_res_and_v_is_refused(lo, dev):
    n = NB + 1
    op = lo.opLDL(dev_matrix(problem(n, np.float64)[0], torch.float64, dev))
    buf = torch.ones(n + 1, dtype=torch.float64, device=dev)
    with pytest.raises(lo.MxloError, match="overlaps"):
        lo.mul(buf[1:], op, buf[:n], 1.0, 0.0)
    assert torch.equal(buf, torch.ones_like(buf))           # nothing was launched


# ------------------------------------------------------------------------------------------------ 7. composition, matrices
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_to_dense_times_k_is_the_identity_and_composition_returns_v(lo, dev, dtype):
    """|X K - I|_2 <= n (n eps rho) |X|_2 |K|_2 with X = to_dense(opLDL(K)): check 1's bound for each of the n columns.
    opLDL(K) * LinearOperator(K): the product K v carries a relative error n eps, the solve turns a relative
    perturbation delta of its right-hand side or matrix into cond(K) delta: |got - v| <= 2 cond(K) n eps rho |v|."""
    n = NB + 1
    K, v, nK, cond, _, _, rho = problem(n, NP[dtype])
    eps = float(torch.finfo(dtype).eps)
    Kd = dev_matrix(K, dtype, dev)
    op = lo.opLDL(Kd)
    X = host(lo.to_dense(op))
    assert np.linalg.norm(X @ K - np.eye(n), 2) <= n * n * eps * rho * np.linalg.norm(X, 2) * nK
    vd = dev_vec(v, dtype, dev)
    got = host(lo.apply(op * lo.LinearOperatorFromMatrix(Kd), vd))
    assert np.linalg.norm(got - v) <= 2 * cond * n * eps * rho * np.linalg.norm(v)


@gpu
def test_mul_on_a_matrix_equals_the_single_applies_bit_for_bit(lo, dev):
    n, dtype = 2 * NB + 1, torch.float64
    op = lo.opLDL(dev_matrix(problem(n, np.float64)[0], dtype, dev))
    rng = np.random.default_rng(8)
    V = dev_matrix(rng.standard_normal((n, 3)), dtype, dev)
    R0 = dev_matrix(rng.standard_normal((n, 3)), dtype, dev)
    for w in (op, lo.transpose(op)):
        R = R0.clone(memory_format=torch.preserve_format)
        lo.mul(R, w, V, 2.0, -0.5)
        for j in range(3):
            r = R0[:, j].clone()
            lo.mul(r, w, V[:, j].clone(), 2.0, -0.5)
            assert torch.equal(R[:, j], r), j


# ------------------------------------------------------------------------------------------------ 8. contract of the hot path
def snap(lo):
    a = (C.c_int64 * 12)()
    lo._lib.call("mxlo_debug_counters", a)
    return dict(zip(NAMES, list(a)))


@gpu
def test_an_apply_is_reproducible_capturable_and_only_launches(lo, dev):
    import gc
    n, dtype = 4 * NB + 3, torch.float64
    K, v = problem(n, np.float64)[:2]
    op = lo.opLDL(dev_matrix(K, dtype, dev))
    nblk = (n + NB - 1) // NB
    vd = dev_vec(v, dtype, dev)
    res0 = torch.linspace(-1, 1, n, dtype=dtype, device=dev)
    runs = []
    for _ in range(2):
        res = res0.clone()
        lo.mul(res, op, vd, 2.0, -0.5)
        runs.append(res)
    assert torch.equal(runs[0], runs[1])
    res = res0.clone()
    g = lo.capture_mul(res, op, vd, 2.0, -0.5)
    res.copy_(res0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(res, runs[0])
    gc.collect()
    torch.cuda.synchronize()
    a = snap(lo)
    lo.mul(res, op, vd, 2.0, -0.5)
    b = snap(lo)
    torch.cuda.synchronize()
    d = {key: b[key] - a[key] for key in NAMES}
    assert d["launch"] == 2 * nblk - 1, d
    assert not {key: x for key, x in d.items() if key != "launch" and x}, d
