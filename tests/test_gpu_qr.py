"""opQR on the device (csrc/linalg.hip, linearoperators.jl_amd/linalg.py): least-squares and minimum-norm solves through an
unpivoted Householder QR, against numpy (LAPACK) in Float64 on the host. The oracle has no rectangular solve.

Matrices. The reference's simple_matrix (test/test_aux.jl:3-17) made rectangular: A = U diag(1 + i/(n-1)) V' with U (m x n)
and V (n x n) from QR of Gaussians of default_rng(7300 + 7 m + n); the condition number is 2 for every shape. A is rounded to the
device precision before anything is computed; v and u are Gaussians, so v is NOT in range(A).

Shapes (mf, nf), the smallest at which the blocking (block columns and row chunks of NB = 64) can go wrong: see SHAPES;
(77, 40) lives in a leading dimension of 79 with NaN in the padding; (40001, 5) has more row chunks than the 512 workgroups a
pass over the rows may use, so they stride, and its odd height leaves no column start 16-byte aligned.

Bound. m eps(T) with m = mf: Higham's normwise backward error of Householder QR and of the least-squares solve through it
(Accuracy and Stability of Numerical Algorithms, Thms 19.4 and 20.3: gamma~_{mn}) with the constants and the factor n
dropped — stricter than the theorem; it is the n eps of the square solve tests when m = n. Derived, not measured; LAPACK's
own QR solve stays at or below 0.23 of it at every shape here in both precisions. Every test prints observed / bound;
the maxima seen on an MI355X are in DESIGN.md §4."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
NB = 64
SHAPES = [(1, 1), (5, 3), (63, 63), (64, 64), (65, 64), (65, 65), (129, 65), (200, 129), (300, 193), (2049, 129), (2049, 1),
          (77, 40), (40001, 5)]
LD = {(77, 40): 79}
IDS = [f"{m}x{n}" for m, n in SHAPES]
DTYPES = [torch.float64, torch.float32]
NP = {torch.float64: np.float64, torch.float32: np.float32}
NAMES = ("malloc", "free", "h2d", "d2h", "d2d", "d2h_bytes", "stream_sync", "device_sync", "event_sync", "memset_async",
         "launch", "blocking_copy")


def simple_matrix(rng, m, n):
    """test/test_aux.jl:3-17 for a real element type and m >= n: U S V' with singular values 1 .. 2 (n = 1: the value 1)"""
    U = np.linalg.qr(rng.standard_normal((m, n)))[0]
    V = np.linalg.qr(rng.standard_normal((n, n)))[0]
    return U @ np.diag(1 + np.arange(n) / max(n - 1, 1)) @ V.T


@functools.lru_cache(maxsize=None)
def problem(m, n, npd):
    """(A, v, u, |A|_2) for the tall m x n case in the precision the device gets, as read-only Float64 arrays"""
    rng = np.random.default_rng(7300 + 7 * m + n)
    A = simple_matrix(rng, m, n).astype(npd).astype(np.float64)
    v = rng.standard_normal(m).astype(npd).astype(np.float64)
    u = rng.standard_normal(n).astype(npd).astype(np.float64)
    for a in (A, v, u):
        a.setflags(write=False)
    return A, v, u, float(np.linalg.norm(A, 2))


def dev_matrix(A, dtype, dev, ld=None, rowmajor=False):
    """A on the device: column-major in a leading dimension ld >= rows (the padding holds NaN), or row-major"""
    t = torch.from_numpy(np.ascontiguousarray(A)).to(dtype).to(dev)
    if rowmajor:
        return t.contiguous()
    ld = ld or max(A.shape[0], 1)
    buf = torch.full((ld * A.shape[1],), float("nan"), dtype=dtype, device=dev)
    out = buf.as_strided(A.shape, (1, ld))
    out.copy_(t)
    return out


def dev_vec(x, dtype, dev):
    return torch.from_numpy(np.asarray(x)).to(dtype).to(dev)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


_OPS = {}


def factored(lo, dev, shape, dtype, wide=False):
    """opQR of the tall problem (or of its transpose, a wide matrix), factored once per case and shared"""
    key = (shape, dtype, wide)
    if key not in _OPS:
        A = problem(*shape, NP[dtype])[0]
        ld = LD.get(shape)
        _OPS[key] = lo.opQR(dev_matrix(A.T, dtype, dev) if wide else dev_matrix(A, dtype, dev, ld))
    return _OPS[key]


def apply(lo, w, x, dtype, dev):
    res = torch.full((lo.size(w, 1),), float("nan"), dtype=dtype, device=dev)
    lo.mul(res, w, dev_vec(x, dtype, dev))
    out = host(res)
    assert np.isfinite(out).all()
    return out


def held(tag, observed, bound):
    print(f"{tag}: {observed:.3e} = {observed / bound:.3e} of the bound")
    assert observed <= bound, (tag, observed / bound)


def lsq_error(A, nA, v, x):
    return float(np.linalg.norm(A.T @ (v - A @ x)) / (nA * (nA * np.linalg.norm(x) + np.linalg.norm(v))))


def minimum_norm_residual(A, nA, u, y):
    return float(np.linalg.norm(A.T @ y - u) / (nA * np.linalg.norm(y)))


def check_least_squares(tag, A, nA, v, x, eps):
    m = A.shape[0]
    held(f"lsq {tag}", lsq_error(A, nA, v, x), m * eps)


def check_minimum_norm(tag, A, nA, u, y, eps):
    m = A.shape[0]
    held(f"minnorm residual {tag}", minimum_norm_residual(A, nA, u, y), m * eps)
    proj = A @ np.linalg.lstsq(A, y, rcond=None)[0]
    held(f"minnorm range {tag}", float(np.linalg.norm(y - proj) / np.linalg.norm(y)), m * eps)


# ------------------------------------------------------------------------------------------------ 1. least squares
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_least_squares_solution_of_a_tall_system(lo, dev, shape, dtype):
    A, v, _, nA = problem(*shape, NP[dtype])
    eps = float(torch.finfo(dtype).eps)
    op = factored(lo, dev, shape, dtype)
    assert tuple(op.shape) == (shape[1], shape[0]) and op._tall
    assert not op.symmetric and not op.hermitian
    check_least_squares(f"op {shape} {dtype}", A, nA, v, apply(lo, op, v, dtype, dev), eps)
    wide = factored(lo, dev, shape, dtype, wide=True)
    assert tuple(wide.shape) == shape and wide._tall == (shape[0] == shape[1])
    check_least_squares(f"transpose(opQR(A')) {shape} {dtype}", A, nA, v, apply(lo, lo.transpose(wide), v, dtype, dev), eps)


# ------------------------------------------------------------------------------------------------ 2. minimum norm
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_minimum_norm_solution_of_a_wide_system(lo, dev, shape, dtype):
    A, _, u, nA = problem(*shape, NP[dtype])
    eps = float(torch.finfo(dtype).eps)
    op = factored(lo, dev, shape, dtype)
    check_minimum_norm(f"transpose(op) {shape} {dtype}", A, nA, u, apply(lo, lo.transpose(op), u, dtype, dev), eps)
    wide = factored(lo, dev, shape, dtype, wide=True)
    check_minimum_norm(f"opQR(A') {shape} {dtype}", A, nA, u, apply(lo, wide, u, dtype, dev), eps)


# ------------------------------------------------------------------------------------------------ 3. the factor
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_r_of_the_factor_reproduces_the_gram_matrix(lo, dev, shape, dtype):
    """R'R = A'A whatever the signs of R's rows are (they are free), so R is not compared with numpy's entry by entry"""
    A, _, _, nA = problem(*shape, NP[dtype])
    m, n = shape
    eps = float(torch.finfo(dtype).eps)
    W = factored(lo, dev, shape, dtype)._factor[0]
    assert tuple(W.shape) == (m, n) and W.stride(0) == 1 and W.stride(1) == m and W.dtype is dtype
    R = np.triu(host(W[:n, :]))
    assert np.isfinite(R).all() and (np.diag(R) != 0).all()
    held(f"R'R {shape} {dtype}", float(np.linalg.norm(R.T @ R - A.T @ A, 2) / nA ** 2), m * eps)


# ------------------------------------------------------------------------------------------------ 4. exact answers
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_scaled_identity_on_zero_rows_is_solved_bit_for_bit(lo, dev, dtype):
    """A = [2 I; 0]: every sub-column is zero, so every tau is 0, H = I and R = 2 I; halving is exact"""
    m, n = 2 * NB + 9, NB + 20
    A = np.zeros((m, n))
    A[:n, :n] = 2 * np.eye(n)
    rng = np.random.default_rng(7)
    v = rng.standard_normal(m).astype(NP[dtype]).astype(np.float64)
    u = rng.standard_normal(n).astype(NP[dtype]).astype(np.float64)
    op = lo.opQR(dev_matrix(A, dtype, dev))
    assert np.array_equal(apply(lo, op, v, dtype, dev), v[:n] / 2)
    assert np.array_equal(apply(lo, lo.transpose(op), u, dtype, dev), np.concatenate([u / 2, np.zeros(m - n)]))


# ------------------------------------------------------------------------------------------------ 5. the reference's criterion
@gpu
@pytest.mark.parametrize("shape", [(10, 6), (6, 10)], ids=["10x6", "6x10"])
def test_the_reference_criterion_made_rectangular(lo, dev, shape):
    """test/test_linop.jl:474-478: |A \\ v - op v| <= sqrt(eps) |v| for op, transpose(op) (with A') and adjoint(op)"""
    dtype = torch.float64
    m, k = shape
    rng = np.random.default_rng(7300 + 7 * m + k)
    A = simple_matrix(rng, m, k) if m >= k else simple_matrix(rng, k, m).T
    v, u = rng.standard_normal(m), rng.standard_normal(k)
    op = lo.opQR(dev_matrix(A, dtype, dev))
    tol = np.sqrt(np.finfo(np.float64).eps)
    for name, w, B, b in (("op", op, A, v), ("transpose", lo.transpose(op), A.T, u), ("adjoint", lo.adjoint(op), A.T, u)):
        want = np.linalg.lstsq(B, b, rcond=None)[0]
        got = apply(lo, w, b, dtype, dev)
        e = np.linalg.norm(want - got)
        print(f"reference criterion {shape} {name}: {e:.3e} against {tol * np.linalg.norm(b):.3e}")
        assert e <= tol * np.linalg.norm(b), (name, e)


# ------------------------------------------------------------------------------------------------ 6. layouts
@gpu
@pytest.mark.parametrize("rowmajor", [False, True], ids=["colmajor", "rowmajor"])
@pytest.mark.parametrize("wide", [False, True], ids=["129x65", "65x129"])
def test_both_storage_orders_of_tall_and_wide_matrices(lo, dev, wide, rowmajor):
    """column-major tall and row-major wide are read as they lie, the other two are transposed while they are copied"""
    dtype, shape = torch.float64, (129, 65)
    A, v, u, nA = problem(*shape, np.float64)
    eps = float(torch.finfo(dtype).eps)
    Ad = dev_matrix(A.T if wide else A, dtype, dev, rowmajor=rowmajor)
    assert (Ad.stride(1) == 1) == rowmajor
    before = Ad.clone()
    op = lo.opQR(Ad)
    assert op._tall == (not wide) and tuple(op.shape) == ((129, 65) if wide else (65, 129))
    lsq, mn = (lo.transpose(op), op) if wide else (op, lo.transpose(op))
    check_least_squares(f"layout wide={wide} rowmajor={rowmajor}", A, nA, v, apply(lo, lsq, v, dtype, dev), eps)
    check_minimum_norm(f"layout wide={wide} rowmajor={rowmajor}", A, nA, u, apply(lo, mn, u, dtype, dev), eps)
    assert torch.equal(Ad, before)                                        # A is not modified, bit for bit


# ------------------------------------------------------------------------------------------------ 7. singular columns
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("fill", ["zero", "nan"])
def test_a_zero_or_non_finite_column_raises_with_its_index(lo, dev, dtype, fill):
    """a zero column stays exactly zero under every reflector, and a column is only ever updated from itself and the
    reflectors, so the NaN of one column reaches no other: the first failing column is this one"""
    m, n, j = 2 * NB + 9, NB + 20, NB + 6
    A = np.array(problem(m, n, NP[dtype])[0])
    if fill == "zero":
        A[:, j] = 0.0
    else:
        A[j:, j] = np.nan
    with pytest.raises(lo.SingularException) as ei:
        lo.opQR(dev_matrix(A, dtype, dev))
    assert ei.value.info == j + 1


# ------------------------------------------------------------------------------------------------ 8. alpha, beta, NaN, aliasing
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(129, 65), (65, 65)], ids=["129x65", "65x65"])
def test_alpha_beta_against_numpy_and_nan_in_res_with_beta_zero(lo, dev, shape, dtype):
    """v = A x0 is consistent, so the residual term of the least-squares forward bound vanishes and the forward error of x is
    kappa m eps |x| normwise (kappa = 2 by construction); the 2 eps are the two roundings of the epilogue"""
    A, _, _, _ = problem(*shape, NP[dtype])
    m, n = shape
    eps = float(torch.finfo(dtype).eps)
    rng = np.random.default_rng(11)
    x0 = rng.standard_normal(n)
    v = (A @ x0).astype(NP[dtype]).astype(np.float64)
    x = np.linalg.lstsq(A, v, rcond=None)[0]
    res0 = rng.standard_normal(n).astype(NP[dtype]).astype(np.float64)
    op = factored(lo, dev, shape, dtype)
    vd = dev_vec(v, dtype, dev)
    alpha, beta = 2.0, -0.5
    res = dev_vec(res0, dtype, dev)
    lo.mul(res, op, vd, alpha, beta)
    err = np.linalg.norm(host(res) - (alpha * x + beta * res0))
    bound = (2 * m * eps + 2 * eps) * (abs(alpha) * np.linalg.norm(x) + abs(beta) * np.linalg.norm(res0))
    held(f"alpha beta {shape} {dtype}", float(err), float(bound))
    res = torch.full((n,), float("nan"), dtype=dtype, device=dev)
    lo.mul(res, op, vd, alpha, 0.0)
    assert np.isfinite(host(res)).all()
    held(f"beta = 0 {shape} {dtype}", float(np.linalg.norm(host(res) - alpha * x)), float((2 * m * eps + 2 * eps) * abs(alpha) * np.linalg.norm(x)))
    res = torch.full((m,), float("nan"), dtype=dtype, device=dev)         # the other mode writes all mf entries
    lo.mul(res, lo.transpose(op), dev_vec(res0, dtype, dev), alpha, 0.0)
    assert np.isfinite(host(res)).all()


@gpu
@pytest.mark.parametrize("n", [5, NB + 1])
def test_res_may_be_v_for_a_square_matrix(lo, dev, n):
    dtype = torch.float64
    A, v, _, _ = problem(n, n, np.float64)
    eps = np.finfo(np.float64).eps
    op = lo.opQR(dev_matrix(A, dtype, dev))
    x = np.linalg.solve(A, v)
    for w, want in ((op, x), (lo.transpose(op), np.linalg.solve(A.T, v))):
        xv = dev_vec(v, dtype, dev)
        lo.mul(xv, w, xv, 2.0, -0.5)
        bound = (2 * n * eps + 2 * eps) * (2.0 * np.linalg.norm(want) + 0.5 * np.linalg.norm(v))
        held(f"res is v n={n}", float(np.linalg.norm(host(xv) - (2.0 * want - 0.5 * v))), float(bound))


@gpu
def test_partial_overlap_of_res_and_v_is_refused(lo, dev):
    n = NB + 1
    op = lo.opQR(dev_matrix(problem(n, n, np.float64)[0], torch.float64, dev))
    buf = torch.ones(n + 1, dtype=torch.float64, device=dev)
    for w in (op, lo.transpose(op)):
        with pytest.raises(lo.MxloError, match="overlaps"):
            lo.mul(buf[1:], w, buf[:n], 1.0, 0.0)
        assert torch.equal(buf, torch.ones_like(buf))                     # nothing was launched
    tall = factored(lo, dev, (129, 65), torch.float64)                    # a rectangular operator: res may not even BE v's memory
    big = torch.ones(129, dtype=torch.float64, device=dev)
    with pytest.raises(lo.MxloError, match="overlaps"):
        lo.mul(big[:65], tall, big, 1.0, 0.0)
    assert torch.equal(big, torch.ones_like(big))


# ------------------------------------------------------------------------------------------------ 9. contract of the hot path
def counters(lo):
    a = (C.c_int64 * 12)()
    lo._lib.call("mxlo_debug_counters", a)
    return dict(zip(NAMES, list(a)))


@gpu
def test_an_apply_is_reproducible_capturable_and_only_launches(lo, dev):
    import gc
    dtype = torch.float64
    deltas = []
    for shape in ((129, 65), (2049, 65)):
        m, n = shape
        A, v, u, _ = problem(m, n, np.float64)
        op = factored(lo, dev, shape, dtype)
        for w, x, nres in ((op, v, n), (lo.transpose(op), u, m)):
            xd = dev_vec(x, dtype, dev)
            res0 = torch.linspace(-1, 1, nres, dtype=dtype, device=dev)
            runs = []
            for _ in range(2):
                res = res0.clone()
                lo.mul(res, w, xd, 2.0, -0.5)
                runs.append(res)
            assert torch.equal(runs[0], runs[1])
            res = res0.clone()
            g = lo.capture_mul(res, w, xd, 2.0, -0.5)
            res.copy_(res0)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(res, runs[0])
            gc.collect()
            torch.cuda.synchronize()
            a = counters(lo)
            lo.mul(res, w, xd, 2.0, -0.5)
            b = counters(lo)
            torch.cuda.synchronize()
            d = {key: b[key] - a[key] for key in NAMES}
            assert d["launch"] == lo.linalg.qr_launches(n), d
            assert not {key: x for key, x in d.items() if key != "launch" and x}, d
            deltas.append(d["launch"])
    assert len(set(deltas)) == 1, deltas                                  # the same for 129 and 2049 rows, in both modes


# ------------------------------------------------------------------------------------------------ 10. matrix operand
@gpu
def test_a_matrix_operand_equals_its_columns_bit_for_bit(lo, dev):
    dtype, shape = torch.float64, (129, 65)
    m, n = shape
    op = factored(lo, dev, shape, dtype)
    rng = np.random.default_rng(13)
    for w, nin, nout in ((op, m, n), (lo.transpose(op), n, m)):
        V = torch.from_numpy(rng.standard_normal((3, nin))).to(dtype).to(dev).t()      # column-major nin x 3
        R0 = torch.from_numpy(rng.standard_normal((3, nout))).to(dtype).to(dev).t()
        R = R0.clone(memory_format=torch.preserve_format)
        lo.mul(R, w, V, 2.0, -0.5)
        for j in range(3):
            r = R0[:, j].clone()
            lo.mul(r, w, V[:, j].clone(), 2.0, -0.5)
            assert torch.equal(R[:, j], r), j
