"""opCholesky and triangular opInverse on the device (csrc/linalg.hip, linearoperators.jl_amd/linalg.py) against numpy
(LAPACK) in Float64 on the host. The oracle has no solve.

Matrices. SPD: M = G G' + I with G = randn(n, n) / sqrt(n), symmetrised, seeded (condition number about 5 for every n
used here). Triangular: the numpy Cholesky factor of such an M (lower) and its transpose (upper) — random triangular
matrices are exponentially ill-conditioned and are not used.

Sizes: the smallest at which the blocking (block columns of NB = 64) can go wrong — 1, 5, NB - 1, NB, NB + 1, 2 NB + 1,
77 in a leading dimension of 79 (no multiple of 16 bytes in either precision, ld > n), and 2049 (33 block columns, the
last one a single column).

Backward error bound. eta = |A x - v|_2 / (|A|_2 |x|_2) <= n eps(T): the normwise bound for substitution and for a
Cholesky solve (Higham, Accuracy and Stability of Numerical Algorithms, Thms 8.5 and 10.4, constants dropped). It is
derived, not measured. A is the matrix the device sees (the Float32 rounding of it for Float32), x the device's result, both
taken to Float64 on the host."""
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
ETA_MAX = {}                                    # observed maxima of eta / (n eps), per dtype (printed by the tests)


@functools.lru_cache(maxsize=None)
def problem(n, npd):
    """(M, L, |M|_2, v) in the precision the device gets, as Float64 arrays; computed once per (n, dtype), read-only."""
    rng = np.random.default_rng(4200 + n)
    G = rng.standard_normal((n, n)) / np.sqrt(n)
    M = G @ G.T + np.eye(n)
    M = ((M + M.T) / 2).astype(npd).astype(np.float64)
    L = np.linalg.cholesky(M).astype(npd).astype(np.float64)
    v = rng.standard_normal(n).astype(npd).astype(np.float64)
    for a in (M, L, v):
        a.setflags(write=False)
    return M, L, float(np.linalg.eigvalsh(M)[-1]), v


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


def build(lo, kind, n, dtype, dev, rowmajor=False):
    """(operator, matrix A it inverts, |A|_2, device matrix) for kind in chol / lower / upper"""
    M, L, nM, _ = problem(n, NP[dtype])
    if kind == "chol":
        Md = dev_matrix(M, dtype, dev, LD.get(n), rowmajor)
        return lo.opCholesky(Md), M, nM, Md
    A = L if kind == "lower" else np.ascontiguousarray(L.T)
    Ad = dev_matrix(A, dtype, dev, LD.get(n), rowmajor)
    return lo.opInverse(Ad), A, float(np.sqrt(nM)), Ad          # |L|_2 = sqrt(|L L'|_2)


# ------------------------------------------------------------------------------------------------ 1. backward error
@gpu
@pytest.mark.parametrize("kind", ["chol", "lower", "upper"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", NS)
def test_backward_error_of_the_solve_and_of_its_transpose_and_adjoint(lo, dev, n, dtype, kind):
    op, A, nA, _ = build(lo, kind, n, dtype, dev)
    v = problem(n, NP[dtype])[3]
    vd = dev_vec(v, dtype, dev)
    eps = float(torch.finfo(dtype).eps)
    for name, w, At in (("op", op, A), ("transpose", lo.transpose(op), A.T), ("adjoint", lo.adjoint(op), A.T)):
        res = torch.full((n,), float("nan"), dtype=dtype, device=dev)
        lo.mul(res, w, vd)
        x = host(res)
        assert np.isfinite(x).all(), (name, n)
        e = eta(At, nA, x, v)
        ETA_MAX[dtype] = max(ETA_MAX.get(dtype, 0.0), e / (n * eps))
        print(f"eta {kind} {name} n={n} {dtype}: {e:.3e} = {e / (n * eps):.3e} n eps")
        # n * eps(T): derived (module docstring). Observed maximum of eta / (n eps) on an MI355X: see DESIGN.md §4
        assert e <= n * eps, (kind, name, n, dtype, e / (n * eps))


@gpu
@pytest.mark.parametrize("kind", ["chol", "lower", "upper"])
def test_row_major_matrices_are_read_in_place(lo, dev, kind):
    """torch's default layout: the column-major storage of the transpose (opInverse swaps N and T, opCholesky reads the
    other triangle of the storage)."""
    n, dtype = 2 * NB + 1, torch.float64
    op, A, nA, Ad = build(lo, kind, n, dtype, dev, rowmajor=True)
    assert Ad.stride(1) == 1
    v = problem(n, np.float64)[3]
    vd = dev_vec(v, dtype, dev)
    for w, At in ((op, A), (lo.transpose(op), A.T)):
        x = host(lo.apply(w, vd))
        assert eta(At, nA, x, v) <= n * np.finfo(np.float64).eps
    if kind != "chol":
        assert op._factor[0].data_ptr() == Ad.data_ptr()            # aliased, not copied
        assert op._triangle == kind


# ------------------------------------------------------------------------------------------------ 2. the reference's criterion
def simple_matrix(rng, n):
    """test/test_aux.jl:3-17 for a real element type: U S V' with singular values 1 .. 2"""
    U = np.linalg.qr(rng.random((n, n)))[0]
    V = np.linalg.qr(rng.random((n, n)))[0]
    return U @ np.diag(1 + np.arange(n) / (n - 1)) @ V.T


@gpu
def test_reference_criterion_of_test_linop(lo, dev):
    """test/test_linop.jl:474-487: |B \\ v - Binv v| <= sqrt(eps) |v| for Binv, transpose(Binv), Binv' with B = A'A, n = 10;
    the same for the inverse of a triangular matrix."""
    n, rtol = 10, np.sqrt(np.finfo(np.float64).eps)
    rng = np.random.default_rng(10)
    A = simple_matrix(rng, n)
    B = A.T @ A
    v = rng.random(n)
    vd = dev_vec(v, torch.float64, dev)
    Binv = lo.opCholesky(dev_matrix(B, torch.float64, dev))
    for w, Bt in ((Binv, B), (lo.transpose(Binv), B.T), (lo.adjoint(Binv), B.T)):
        assert np.linalg.norm(np.linalg.solve(Bt, v) - host(lo.apply(w, vd))) <= rtol * np.linalg.norm(v)
    L = np.linalg.cholesky(B)
    for T in (L, np.ascontiguousarray(L.T)):
        Tinv = lo.opInverse(dev_matrix(T, torch.float64, dev))
        for w, Tt in ((Tinv, T), (lo.transpose(Tinv), T.T), (lo.adjoint(Tinv), T.T)):
            assert np.linalg.norm(np.linalg.solve(Tt, v) - host(lo.apply(w, vd))) <= rtol * np.linalg.norm(v)


# ------------------------------------------------------------------------------------------------ 3. alpha and beta
@gpu
@pytest.mark.parametrize("kind", ["chol", "lower", "upper"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_alpha_beta_nan_in_res_and_res_is_v(lo, dev, dtype, kind):
    """Against alpha * x_numpy + beta * res0. Tolerance: the forward error of a solve with backward error n eps is at most
    cond(A) n eps |x| (first order), the epilogue adds one rounding of each term:
    |got - want| <= (cond(A) n eps + 2 eps) (|alpha| |x| + |beta| |res0|)."""
    n = 2 * NB + 1
    op, A, nA, _ = build(lo, kind, n, dtype, dev)
    v = problem(n, NP[dtype])[3]
    eps = float(torch.finfo(dtype).eps)
    x = np.linalg.solve(A, v)
    rel = np.linalg.cond(A) * n * eps + 2 * eps
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
        xv = vd.clone()                                     # res is v: alpha F^{-1} v + beta v
        lo.mul(xv, op, xv, a, b)
        tol = rel * (abs(a) * np.linalg.norm(x) + abs(b) * np.linalg.norm(v))
        assert np.linalg.norm(host(xv) - (a * x + b * v)) <= tol, (a, b)


@gpu
def test_partial_overlap_of_res_and_v_is_refused(lo, dev):
    n = NB + 1
    op = build(lo, "chol", n, torch.float64, dev)[0]
    buf = torch.ones(n + 1, dtype=torch.float64, device=dev)
    with pytest.raises(lo.MxloError, match="overlaps"):
        lo.mul(buf[1:], op, buf[:n], 1.0, 0.0)
    assert torch.equal(buf, torch.ones_like(buf))           # nothing was launched


# ------------------------------------------------------------------------------------------------ 4. refusals
@gpu
def test_check_true_refuses_non_symmetric_and_negative_definite(lo, dev):
    rng = np.random.default_rng(5)
    A = simple_matrix(rng, 5)                               # test/test_linop.jl:489
    with pytest.raises(lo.LinearOperatorException, match="not Hermitian"):
        lo.opCholesky(dev_matrix(A, torch.float64, dev), check=True)
    S = -(A @ A.T)
    with pytest.raises(lo.LinearOperatorException, match="not positive definite"):
        lo.opCholesky(dev_matrix(S, torch.float64, dev), check=True)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_quasi_definite_matrix_raises_posdef_with_numpys_index(lo, dev, dtype):
    """test/test_linop.jl:491-498: K = [A B'; B -C] is symmetric quasi-definite; the failing leading minor is the first one
    numpy's Cholesky refuses."""
    rng = np.random.default_rng(6)
    U = np.linalg.qr(rng.random((3, 3)))[0]
    A = U @ np.diag([1.0, 1.5, 2.0]) @ U.T
    B = simple_matrix(rng, 3)[:2]
    Q = np.linalg.qr(rng.random((2, 2)))[0]
    Cm = Q @ np.diag([1.0, 2.0]) @ Q.T
    K = np.block([[A, B.T], [B, -Cm]])
    K = (K + K.T) / 2
    want = None
    for k in range(1, 6):
        try:
            np.linalg.cholesky(K[:k, :k])
        except np.linalg.LinAlgError:
            want = k
            break
    assert want == 4
    with pytest.raises(lo.PosDefException) as e:
        lo.opCholesky(dev_matrix(K, dtype, dev))
    assert e.value.info == want
    # a failure in a later block column: the 1-based index counts from the start of the matrix
    n = 2 * NB + 1
    M = problem(n, NP[dtype])[0].copy()
    M[NB + 6, NB + 6] = -1.0
    with pytest.raises(lo.PosDefException) as e:
        lo.opCholesky(dev_matrix(M, dtype, dev))
    assert e.value.info == NB + 7
    M[NB + 6, NB + 6] = np.nan                              # a pivot that is not finite
    with pytest.raises(lo.PosDefException) as e:
        lo.opCholesky(dev_matrix(M, dtype, dev))
    assert e.value.info == NB + 7


@gpu
def test_opinverse_of_a_full_matrix_is_refused_and_a_diagonal_one_is_lower(lo, dev):
    M = problem(5, np.float64)[0]
    with pytest.raises(lo.LinearOperatorException, match="pivoted LU"):
        lo.opInverse(dev_matrix(M, torch.float64, dev))
    d = np.diag([1.0, 2.0, 4.0])
    op = lo.opInverse(dev_matrix(d, torch.float64, dev))
    assert op._triangle == "lower"
    got = host(lo.apply(op, dev_vec(np.ones(3), torch.float64, dev)))
    assert np.array_equal(got, [1.0, 0.5, 0.25])
    # a zero on the diagonal: Inf / NaN, no exception
    z = np.tril(np.ones((3, 3)))
    z[1, 1] = 0.0
    bad = host(lo.apply(lo.opInverse(dev_matrix(z, torch.float64, dev)), dev_vec(np.ones(3), torch.float64, dev)))
    assert not np.isfinite(bad).all()


# ------------------------------------------------------------------------------------------------ 5. structure
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_cholesky_leaves_m_alone_reads_one_triangle_and_has_the_reference_flags(lo, dev, dtype):
    n = NB + 1
    M, _, _, v = problem(n, NP[dtype])
    Md = dev_matrix(M, dtype, dev, n + 2)
    before = Md.clone()
    op = lo.opCholesky(Md)
    assert torch.equal(Md, before)
    assert op.symmetric and op.hermitian and lo.has_args5(op) and op.size() == (n, n) and op.eltype is dtype
    vd = dev_vec(v, dtype, dev)
    x = lo.apply(op, vd)
    Mn = M.copy()
    Mn[np.tril_indices(n, -1)] = np.nan                     # cholesky(M) = cholesky(Hermitian(M, :U)): the strict lower triangle is not read
    x2 = lo.apply(lo.opCholesky(dev_matrix(Mn, dtype, dev, n + 2)), vd)
    assert torch.equal(x, x2)
    assert lo.nprod(op) == 1 and lo.ntprod(op) == 0
    lo.apply(lo.transpose(op), vd)                          # symmetric: transpose goes to prod!
    assert lo.nprod(op) == 2


@gpu
def test_opinverse_aliases_m_and_counts_like_any_leaf(lo, dev):
    n, dtype = 2 * NB + 1, torch.float64
    op, A, _, Ad = build(lo, "lower", n, dtype, dev)
    assert not op.symmetric and not op.hermitian and lo.has_args5(op) and op.size() == (n, n)
    assert op._factor[0].data_ptr() == Ad.data_ptr()
    vd = dev_vec(problem(n, np.float64)[3], dtype, dev)
    x1 = lo.apply(op, vd)
    t1 = lo.apply(lo.transpose(op), vd)
    Ad.mul_(2.0)                                            # in place: the next apply sees it (scaling by 2 is exact)
    assert torch.equal(lo.apply(op, vd) * 2.0, x1)
    assert torch.equal(lo.apply(lo.transpose(op), vd) * 2.0, t1)
    assert lo.nprod(op) == 2 and lo.ntprod(op) == 2 and lo.nctprod(op) == 0
    lo.apply(lo.adjoint(op), vd)
    assert lo.nctprod(op) == 1
    sy = lo.opInverse(Ad, symm=True, herm=True)             # the caller's flags are taken as given (src/linalg.jl:31)
    assert sy.symmetric and sy.hermitian


# ------------------------------------------------------------------------------------------------ 6. composition, matrices
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_to_dense_times_m_is_the_identity_and_composition_returns_v(lo, dev, dtype):
    """|X M - I|_2 <= n (n eps) |X|_2 |M|_2 with X = to_dense(opCholesky(M)): check 1's bound for each of the n columns.
    opCholesky(M) * LinearOperator(M): the product M v carries a relative error n eps, the solve turns a relative
    perturbation delta of its right-hand side or matrix into cond(M) delta: |got - v| <= 2 cond(M) n eps |v|."""
    n = NB + 1
    M, _, nM, v = problem(n, NP[dtype])
    eps = float(torch.finfo(dtype).eps)
    Md = dev_matrix(M, dtype, dev)
    op = lo.opCholesky(Md)
    X = host(lo.to_dense(op))
    assert np.linalg.norm(X @ M - np.eye(n), 2) <= n * n * eps * np.linalg.norm(X, 2) * nM
    vd = dev_vec(v, dtype, dev)
    got = host(lo.apply(op * lo.LinearOperatorFromMatrix(Md), vd))
    assert np.linalg.norm(got - v) <= 2 * np.linalg.cond(M) * n * eps * np.linalg.norm(v)


@gpu
@pytest.mark.parametrize("kind", ["chol", "lower"])
def test_mul_on_a_matrix_equals_the_single_applies_bit_for_bit(lo, dev, kind):
    n, dtype = 2 * NB + 1, torch.float64
    op = build(lo, kind, n, dtype, dev)[0]
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


# ------------------------------------------------------------------------------------------------ 7. contract of the hot path
def snap(lo):
    a = (C.c_int64 * 12)()
    lo._lib.call("mxlo_debug_counters", a)
    return dict(zip(NAMES, list(a)))


@gpu
@pytest.mark.parametrize("kind", ["chol", "lower", "upper"])
def test_an_apply_is_reproducible_capturable_and_only_launches(lo, dev, kind):
    import gc
    n, dtype = 4 * NB + 3, torch.float64
    op = build(lo, kind, n, dtype, dev)[0]
    nblk = (n + NB - 1) // NB
    vd = dev_vec(problem(n, np.float64)[3], dtype, dev)
    res0 = torch.linspace(-1, 1, n, dtype=dtype, device=dev)
    for w in (op, lo.transpose(op)):
        runs = []
        for _ in range(2):
            res = res0.clone()
            lo.mul(res, w, vd, 2.0, -0.5)
            runs.append(res)
        assert torch.equal(runs[0], runs[1])
        res = res0.clone()
        g = lo.capture_mul(res, w, vd, 2.0, -0.5)
        res.copy_(res0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(res, runs[0])
        gc.collect()
        torch.cuda.synchronize()
        a = snap(lo)
        lo.mul(res, w, vd, 2.0, -0.5)
        b = snap(lo)
        torch.cuda.synchronize()
        d = {key: b[key] - a[key] for key in NAMES}
        assert d["launch"] == (2 * nblk - 1 if kind == "chol" else nblk), d
        assert not {key: x for key, x in d.items() if key != "launch" and x}, d
