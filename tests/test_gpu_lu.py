"""opLU on the device (csrc/linalg.hip, linearoperators.jl_amd/linalg.py): the inverse of a general dense matrix through a
partially pivoted LU, against numpy (LAPACK) in Float64 on the host. The oracle has no solve.

Matrices. (a) The reference's simple_matrix (test/test_aux.jl:3-17): U S V' with singular values 1 .. 2 from
default_rng(6200 + n), rounded to the device precision: condition number 2, and LAPACK interchanges nearly every row
(2037 of the 2049 interchanges have ipiv[i] != i at n = 2049; the permutation they compose moves more rows, perm[i] != i).
(b) The SPD matrix G G' + I of test_gpu_linalg.py with its rows rolled down by NB + 1: the large entries sit NB + 1 rows below the diagonal, so the pivots of every panel that ends before column n - NB - 1 come from below
the panel's own 64 x 64 diagonal block — a search confined to that block fails on it. (In the last NB + 1 columns the large
entries are in the rows that wrapped round to the top.)

Sizes: those of test_gpu_linalg.py, the smallest at which the blocking (block columns of NB = 64) can go wrong — 1, 5,
NB - 1, NB, NB + 1, 2 NB + 1, 77 in a leading dimension of 79 with NaN in the padding, and 2049 (33 block columns, the
last one a single column); family (b) at 2 NB + 1 and 4 NB + 3.

Backward error bound. eta = |A x - v|_inf / (|A|_inf |x|_inf) <= n eps(T): the bound for a solve by LU with partial
pivoting (Higham, Accuracy and Stability of Numerical Algorithms, Thm 9.4 with 8.5) with the constants and the growth
factor dropped, so it assumes modest growth and holds only for inputs like these. It is derived, not measured; LAPACK in
the same precision reaches at most 0.25 n eps on family (a) (at n = 1), below 0.02 n eps for n >= 63. A is the matrix the
device sees, x the device's result, both taken to Float64 on the host."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
NB = 64
NS = [1, 5, NB - 1, NB, NB + 1, 2 * NB + 1, 77, 2049]
ROLLED = [2 * NB + 1, 4 * NB + 3]
LD = {77: 79}
DTYPES = [torch.float64, torch.float32]
NP = {torch.float64: np.float64, torch.float32: np.float32}
NAMES = ("malloc", "free", "h2d", "d2h", "d2d", "d2h_bytes", "stream_sync", "device_sync", "event_sync", "memset_async",
         "launch", "blocking_copy")


def simple_matrix(rng, n):
    """test/test_aux.jl:3-17 for a real element type: U S V' with singular values 1 .. 2 (n = 1: the single value 1)"""
    U = np.linalg.qr(rng.random((n, n)))[0]
    V = np.linalg.qr(rng.random((n, n)))[0]
    return U @ np.diag(1 + np.arange(n) / max(n - 1, 1)) @ V.T


@functools.lru_cache(maxsize=None)
def problem(n, npd, family="simple"):
    """(A, v, |A|_inf) in the precision the device gets, as Float64 arrays; computed once per case, read-only."""
    rng = np.random.default_rng(6200 + n)
    if family == "simple":
        A = simple_matrix(rng, n)
    else:
        G = rng.standard_normal((n, n)) / np.sqrt(n)
        A = G @ G.T + np.eye(n)
        A = np.roll((A + A.T) / 2, NB + 1, axis=0)
    A = A.astype(npd).astype(np.float64)
    v = rng.standard_normal(n).astype(npd).astype(np.float64)
    for a in (A, v):
        a.setflags(write=False)
    return A, v, float(np.abs(A).sum(axis=1).max())


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


def norm_inf(A):
    return float(np.abs(A).sum(axis=1).max())


def eta_inf(A, nA, x, v):
    nx = np.abs(x).max()
    return float(np.abs(A @ x - v).max() / (nA * nx)) if nx else float(np.abs(v).max())


def check_solves(lo, op, A, nA, v, dtype, dev, tag):
    """the backward error of op, transpose(op) and adjoint(op) on v, each printed and held to n eps"""
    n = A.shape[0]
    eps = float(torch.finfo(dtype).eps)
    vd = dev_vec(v, dtype, dev)
    for name, w, At, nAt in (("op", op, A, nA), ("transpose", lo.transpose(op), A.T, norm_inf(A.T)),
                             ("adjoint", lo.adjoint(op), A.T, norm_inf(A.T))):
        res = torch.full((n,), float("nan"), dtype=dtype, device=dev)
        lo.mul(res, w, vd)
        x = host(res)
        assert np.isfinite(x).all(), (tag, name)
        e = eta_inf(At, nAt, x, v)
        print(f"eta {tag} {name} n={n} {dtype}: {e:.3e} = {e / (n * eps):.3e} n eps")
        # n * eps(T): derived (module docstring). Observed maximum of eta / (n eps) on an MI355X: see DESIGN.md §4
        assert e <= n * eps, (tag, name, n, dtype, e / (n * eps))


CASES = [(n, "simple") for n in NS] + [(n, "rolled") for n in ROLLED]
IDS = [f"{f}-{n}" for n, f in CASES]


# ------------------------------------------------------------------------------------------------ 1. backward error
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,family", CASES, ids=IDS)
def test_backward_error_of_the_solve_and_of_its_transpose_and_adjoint(lo, dev, n, family, dtype):
    A, v, nA = problem(n, NP[dtype], family)
    op = lo.opLU(dev_matrix(A, dtype, dev, LD.get(n)))
    check_solves(lo, op, A, nA, v, dtype, dev, family)


# ------------------------------------------------------------------------------------------------ 2. the factorisation
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,family", CASES, ids=IDS)
def test_perm_is_a_permutation_l_is_bounded_by_one_and_pa_is_lu(lo, dev, n, family, dtype):
    """|L_ij| <= 1 EXACTLY is the partial-pivoting invariant: the multiplier is a quotient by the largest candidate, and
    rounding a quotient of magnitude <= 1 cannot exceed 1. An unpivoted or block-local search breaks it.
    |A[perm] - L U|_inf <= n eps |A|_inf: Higham Thm 9.3, constants and growth dropped like the bound of the solve."""
    A, _, nA = problem(n, NP[dtype], family)
    op = lo.opLU(dev_matrix(A, dtype, dev, LD.get(n)))
    perm = op._perm
    assert perm.dtype is torch.int32 and perm.shape == (n,) and perm.is_cuda
    p = perm.cpu().numpy()
    assert np.array_equal(np.sort(p), np.arange(n))
    W = host(op._factor[0])
    L, U = np.tril(W, -1) + np.eye(n), np.triu(W)
    assert np.abs(L).max() <= 1.0
    eps = float(torch.finfo(dtype).eps)
    r = norm_inf(A[p] - L @ U) / nA
    print(f"|A[perm] - L U| / |A| {family} n={n} {dtype}: {r:.3e} = {r / (n * eps):.3e} n eps; rows moved: {int((p != np.arange(n)).sum())}")
    assert r <= n * eps
    if family == "rolled":
        # Column j's dominant entry lies in row j + NB + 1 while j + NB + 1 < n, and no earlier interchange has moved that
        # row (interchange j' < j touches rows j' and j' + NB + 1 only). So in every panel that ends before column
        # n - NB - 1 each pivot row lies below the panel's diagonal block; there are (n - NB - 1) // NB >= 1 such panels.
        # From column n - NB - 1 on the dominant entries are those of the rows that wrapped round to the top, which the
        # earlier interchanges have brought to just below the diagonal: nothing is claimed for those panels.
        below = (n - NB - 1) // NB
        assert below >= 1
        rows = p[:below * NB].reshape(below, NB)
        assert (rows >= (np.arange(below) * NB + NB)[:, None]).all()


# ------------------------------------------------------------------------------------------------ 3. only pivoting solves these
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_exchange_matrix_gives_v_reversed_exactly(lo, dev, dtype):
    """J has a zero in every diagonal position; with pivoting L = U = I and P = J: every product is with 0 or 1."""
    n = NB + 1
    J = np.fliplr(np.eye(n))
    v = problem(n, NP[dtype])[1]
    op = lo.opLU(dev_matrix(J, dtype, dev))
    assert np.array_equal(op._perm.cpu().numpy(), np.arange(n)[::-1])
    vd = dev_vec(v, dtype, dev)
    for w in (op, lo.transpose(op)):
        assert np.array_equal(host(lo.apply(w, vd)), v[::-1])


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_zero_in_the_first_diagonal_position_is_pivoted_away(lo, dev, dtype):
    n = NB + 1
    A, v, _ = problem(n, NP[dtype])
    A = A.copy()
    A[0, 0] = 0.0
    assert np.linalg.cond(A) < 100                         # still a well-conditioned matrix; no LU without interchanges
    op = lo.opLU(dev_matrix(A, dtype, dev))
    assert op._perm[0].item() != 0
    check_solves(lo, op, A, norm_inf(A), v, dtype, dev, "a00=0")


# ------------------------------------------------------------------------------------------------ 4. singular, not finite
def same_bits(t, before):
    bits = {torch.float64: torch.int64, torch.float32: torch.int32}[t.dtype]    # same element size: any stride may be viewed
    return torch.equal(t.view(bits), before.view(bits))


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_two_equal_rows_raise_singular_exception(lo, dev, dtype):
    """n = NB, one panel, where the zero pivot is EXACT: two equal rows stay bitwise equal under the same eliminations until
    one of them becomes the pivot row; the other then gets the multiplier 1 and a - 1 * a = 0 in every remaining column.
    That zero row is never chosen while another candidate is non-zero, so it is the last pivot: info = n. (Across block
    columns the trailing update sums in another order and the difference is rounding noise, as in LAPACK.)"""
    n = NB
    A = problem(n, NP[dtype])[0].copy()
    A[NB // 2 + 3] = A[4]
    Md = dev_matrix(A, dtype, dev, n + 2)
    before = Md.clone(memory_format=torch.preserve_format)
    with pytest.raises(lo.SingularException) as e:
        lo.opLU(Md)
    assert e.value.info == n
    assert same_bits(Md, before)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_zero_or_nan_column_raises_with_its_index_counted_from_the_start(lo, dev, dtype):
    """A zero column stays exactly zero under interchanges and updates (0 - l * 0), so every candidate of column NB + 6 is
    zero: info = NB + 7, found by the second panel. With NaN at and below the diagonal of that column the NaN stays in that
    column until it is searched, where NaN wins and is not finite: the same info."""
    n, c = 2 * NB + 1, NB + 6
    A = problem(n, NP[dtype])[0].copy()
    A[:, c] = 0.0
    for fill in (0.0, np.nan):
        A[c:, c] = fill
        Md = dev_matrix(A, dtype, dev)
        before = Md.clone(memory_format=torch.preserve_format)
        with pytest.raises(lo.SingularException) as e:
            lo.opLU(Md)
        assert e.value.info == c + 1, fill
        assert same_bits(Md, before)


# ------------------------------------------------------------------------------------------------ 5. alpha, beta, aliasing
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_alpha_beta_nan_in_res_and_res_is_v(lo, dev, dtype):
    """Against alpha * x_numpy + beta * res0, with the tolerance of test_gpu_linalg.py's test of the same name: the forward
    error of a solve with backward error n eps is at most cond(A) n eps |x| (first order), the epilogue adds one rounding of
    each term: |got - want| <= (cond(A) n eps + 2 eps) (|alpha| |x| + |beta| |res0|)."""
    n = 2 * NB + 1
    A, v, _ = problem(n, NP[dtype])
    op = lo.opLU(dev_matrix(A, dtype, dev))
    eps = float(torch.finfo(dtype).eps)
    rel = np.linalg.cond(A) * n * eps + 2 * eps
    rng = np.random.default_rng(3)
    res0 = rng.standard_normal(n).astype(NP[dtype]).astype(np.float64)
    vd = dev_vec(v, dtype, dev)
    for w, At in ((op, A), (lo.transpose(op), A.T)):
        x = np.linalg.solve(At, v)
        for a, b in ((1.0, 0.0), (2.5, 0.0), (1.0, -0.5), (0.0, 3.0)):
            res = dev_vec(res0, dtype, dev)
            lo.mul(res, w, vd, a, b)
            tol = rel * (abs(a) * np.linalg.norm(x) + abs(b) * np.linalg.norm(res0))
            assert np.linalg.norm(host(res) - (a * x + b * res0)) <= tol, (a, b)
            if b == 0:                                          # beta == 0: res is not read
                res = torch.full((n,), float("nan"), dtype=dtype, device=dev)
                lo.mul(res, w, vd, a, b)
                assert np.isfinite(host(res)).all()
                assert np.linalg.norm(host(res) - a * x) <= rel * abs(a) * np.linalg.norm(x)
            xv = vd.clone()                                     # res is v: alpha A^{-1} v + beta v
            lo.mul(xv, w, xv, a, b)
            tol = rel * (abs(a) * np.linalg.norm(x) + abs(b) * np.linalg.norm(v))
            assert np.linalg.norm(host(xv) - (a * x + b * v)) <= tol, (a, b)


@gpu
def test_res_is_v_inside_one_workgroup(lo, dev):
    """n <= NB: gather, both products and the scattering epilogue are one launch of one workgroup"""
    n, dtype = 5, torch.float64
    A, v, _ = problem(n, np.float64)
    op = lo.opLU(dev_matrix(A, dtype, dev))
    for w, At in ((op, A), (lo.transpose(op), A.T)):
        x = np.linalg.solve(At, v)
        xv = dev_vec(v, dtype, dev)
        lo.mul(xv, w, xv, 2.0, -0.5)
        rel = np.linalg.cond(A) * n * np.finfo(np.float64).eps + 2 * np.finfo(np.float64).eps
        assert np.linalg.norm(host(xv) - (2.0 * x - 0.5 * v)) <= rel * (2.0 * np.linalg.norm(x) + 0.5 * np.linalg.norm(v))


@gpu
def test_partial_overlap_of_res_and_v_is_refused(lo, dev):
    n = NB + 1
    op = lo.opLU(dev_matrix(problem(n, np.float64)[0], torch.float64, dev))
    buf = torch.ones(n + 1, dtype=torch.float64, device=dev)
    for w in (op, lo.transpose(op)):
        with pytest.raises(lo.MxloError, match="overlaps"):
            lo.mul(buf[1:], w, buf[:n], 1.0, 0.0)
        assert torch.equal(buf, torch.ones_like(buf))           # nothing was launched


# ------------------------------------------------------------------------------------------------ 6. row-major M, structure
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_row_major_m_is_read_in_place_and_the_operator_counts_like_a_leaf(lo, dev, dtype):
    """torch's default layout is the column-major storage of the transpose: that storage is factored, N and T swapped"""
    n = 2 * NB + 1
    A, v, nA = problem(n, NP[dtype])
    Md = dev_matrix(A, dtype, dev, rowmajor=True)
    assert Md.stride(1) == 1
    before = Md.clone()
    op = lo.opLU(Md)
    assert torch.equal(Md, before)
    assert not op.symmetric and not op.hermitian and lo.has_args5(op) and op.size() == (n, n) and op.eltype is dtype
    W = host(op._factor[0])                                 # the factors of the storage as it lies: of A'
    p = op._perm.cpu().numpy()
    eps = float(torch.finfo(dtype).eps)
    assert norm_inf(A.T[p] - (np.tril(W, -1) + np.eye(n)) @ np.triu(W)) <= n * eps * norm_inf(A.T)
    check_solves(lo, op, A, nA, v, dtype, dev, "row-major")
    assert lo.nprod(op) == 1 and lo.ntprod(op) == 1 and lo.nctprod(op) == 1
    sy = lo.opLU(Md, symm=True, herm=True)                  # the caller's flags are taken as given (src/linalg.jl:31)
    assert sy.symmetric and sy.hermitian


# ------------------------------------------------------------------------------------------------ 7. the reference's criterion
@gpu
def test_reference_criterion_of_test_linop(lo, dev):
    """test/test_linop.jl:475-478: |A \\ v - Ainv v| <= sqrt(eps) |v| for Ainv, transpose(Ainv), Ainv' at n = 10"""
    n, rtol = 10, np.sqrt(np.finfo(np.float64).eps)
    rng = np.random.default_rng(10)
    A = simple_matrix(rng, n)
    v = rng.random(n)
    vd = dev_vec(v, torch.float64, dev)
    Ainv = lo.opLU(dev_matrix(A, torch.float64, dev))
    for w, At in ((Ainv, A), (lo.transpose(Ainv), A.T), (lo.adjoint(Ainv), A.T)):
        assert np.linalg.norm(np.linalg.solve(At, v) - host(lo.apply(w, vd))) <= rtol * np.linalg.norm(v)


# ------------------------------------------------------------------------------------------------ 8. matrices
@gpu
def test_mul_on_a_matrix_equals_the_single_applies_bit_for_bit(lo, dev):
    n, dtype = 2 * NB + 1, torch.float64
    op = lo.opLU(dev_matrix(problem(n, np.float64)[0], dtype, dev))
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


# ------------------------------------------------------------------------------------------------ 9. contract of the hot path
def snap(lo):
    a = (C.c_int64 * 12)()
    lo._lib.call("mxlo_debug_counters", a)
    return dict(zip(NAMES, list(a)))


@gpu
def test_an_apply_is_reproducible_capturable_and_only_launches(lo, dev):
    import gc
    n, dtype = 4 * NB + 3, torch.float64
    A, v, _ = problem(n, np.float64, "rolled")
    op = lo.opLU(dev_matrix(A, dtype, dev))
    nblk = (n + NB - 1) // NB
    vd = dev_vec(v, dtype, dev)
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
        assert d["launch"] == 2 * nblk - 1, d
        assert not {key: x for key, x in d.items() if key != "launch" and x}, d

