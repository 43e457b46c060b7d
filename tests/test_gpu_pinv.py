"""opPinv(A) on the device (csrc/linalg.hip, linearoperators.jl_amd/linalg.py): the pseudo-inverse of a rank-deficient matrix through
the pivoted QR completed to an orthogonal decomposition, against numpy / scipy in Float64 on the host. The oracle has no
rectangular solve.

Inputs: deficient(), problem_def(), dev_matrix() (NaN in the padding) and the shapes of test_gpu_qrp.py, with (17, 9, 5) as the
smallest case in place of (5, 3, 2): at 5 x 3 the bound 5 eps sits at the floor of the host's own SVD basis. v (mf entries) is
problem_def's; u (nf entries) is Gaussian from default_rng(9700 + 7 mf + nf + U_SEED_OFFSET) and NOT consistent.

Metrics, all relative: lsq_error(F, |F|, v, x) for x = F⁺ v; lsq_error(F', |F|, u, y) for y = (F⁺)' u — the basic solve of
opQR(pivot=True) fails this one for an inconsistent u; the distance of x from the row space of F and of y from range(F),
|x - B B' x| / |x| with B the singular vectors above the gap. A least-squares solution in the row space is THE minimum-norm one.

Bound: mf eps(T) for all four, the derived bound of test_gpu_qr.py and test_gpu_qrp.py (Higham, Thms 19.4 and 20.3 with the
constants and the factor n dropped); the second orthogonal factor adds a backward-stable stage of the same form. Derived, not
measured. test_the_reference_algorithm_and_the_basic_solution (CPU) runs the same two-stage algorithm in the working precision
with scipy and asserts it stays at or below 0.35 of the bound at every case, so a correct device result has a factor of about 3
to spare. Every test prints observed / bound; the maxima seen on an MI355X are in DESIGN.md §4."""
import functools
import gc

import numpy as np
import pytest
import torch

import test_gpu_qrp as q
from test_gpu_qrp import NP, counters, dev_matrix, dev_vec, held, host, lsq_error, problem_def

gpu = pytest.mark.gpu
SHAPES = [(17, 9, 5), (65, 64, 63), (65, 65, 1), (64, 64, 32), (129, 65, 64), (200, 129, 65), (300, 193, 128), (2049, 129, 100),
          (77, 40, 17), (40001, 5, 3)]
LD = {(77, 40, 17): 79}
IDS = [f"{m}x{n}r{r}" for m, n, r in SHAPES]
DTYPES = [torch.float64, torch.float32]
DIDS = ["f64", "f32"]
# the seed of u is 9700 + 7 mf + nf plus this offset; none was needed: the host algorithm stays at or below 0.35 of the bound at
# every case with offset 0 (test_the_reference_algorithm_and_the_basic_solution prints the ratios)
U_SEED_OFFSET = {}


@functools.lru_cache(maxsize=None)
def rhs_u(m, n, r, npd):
    rng = np.random.default_rng(9700 + 7 * m + n + U_SEED_OFFSET.get(((m, n, r), npd), 0))
    u = rng.standard_normal(n).astype(npd).astype(np.float64)
    return q.frozen(u)[0]


def space_distance(M, x):
    """|x - B B' x| / |x|, B an orthonormal basis of range(M)"""
    Mc = np.ascontiguousarray(M)
    B = q.range_basis(Mc.tobytes(), Mc.shape)
    return float(np.linalg.norm(x - B @ (B.T @ x)) / np.linalg.norm(x))


def four_metrics(F, nF, v, u, x, y):
    """(lsq of x, lsq of y, distance of x from the row space of F, distance of y from range(F))"""
    return (lsq_error(F, nF, v, x), lsq_error(F.T, nF, u, y), space_distance(F.T, x), space_distance(F, y))


def host_cod(F, npd, rtol=None):
    """the device's algorithm on the host in the precision npd: geqp3, the rank rule (rtol: None for the default max(m, n) eps),
    QR of [R11 R12]'; (rank, solve, solve_t)"""
    from scipy.linalg import qr, solve_triangular
    m, n = F.shape
    Q1, R, perm = qr(F.astype(npd), mode="economic", pivoting=True)
    d = np.abs(np.diag(R)).astype(np.float64)
    ok = d > (max(m, n) * float(np.finfo(npd).eps) if rtol is None else rtol) * d[0]
    r = int(n if ok.all() else np.argmin(ok))
    Q2, R2 = qr(np.ascontiguousarray(R[:r, :].T), mode="economic")

    def solve(v):
        x = np.zeros(n, dtype=npd)
        x[perm] = Q2 @ solve_triangular(R2, Q1[:, :r].T @ v.astype(npd), trans="T")
        return x.astype(np.float64)

    def solve_t(u):
        return (Q1[:, :r] @ solve_triangular(R2, Q2.T @ u.astype(npd)[perm])).astype(np.float64)

    return r, solve, solve_t


# ------------------------------------------------------------------------------------------------ 0. the inputs (CPU)
@pytest.mark.parametrize("npd", [np.float64, np.float32], ids=DIDS)
def test_the_reference_algorithm_and_the_basic_solution(npd):
    """The two-stage algorithm on the host, in the working precision, is at or below 0.35 of the bound mf eps in all four metrics
    at every case; LAPACK's BASIC solution of the same inputs is at least 30 bounds away from the row space wherever r < nf, so
    the row-space metric tells the two apart."""
    eps = float(np.finfo(npd).eps)
    worst, nearest = 0.0, np.inf
    for shape in SHAPES:
        m, n, r = shape
        F, v, nF = problem_def(*shape, npd)
        u = rhs_u(*shape, npd)
        rank, solve, solve_t = host_cod(F, npd)
        assert rank == r, (shape, rank)
        e = np.array(four_metrics(F, nF, v, u, solve(v), solve_t(u))) / (m * eps)
        print(f"host cod {shape} {npd.__name__}: {e[0]:.3f} {e[1]:.3f} {e[2]:.3f} {e[3]:.3f} of the bound")
        assert e.max() <= 0.35, (shape, e)
        worst = max(worst, float(e.max()))
        rb, _, _, basic, _ = q.lapack_basic(F, npd)
        assert rb == r
        if r < n:
            far = space_distance(F.T, basic(v)) / (m * eps)
            print(f"basic solution {shape} {npd.__name__}: {far:.3e} bounds from the row space")
            assert far >= 30, (shape, far)
            nearest = min(nearest, far)
    print(f"host cod {npd.__name__}: worst {worst:.3f} of the bound; the basic solution at least {nearest:.1f} bounds away")


# ------------------------------------------------------------------------------------------------ the shared operators
_OPS = {}


def factored(lo, dev, shape, dtype, wide=False):
    """opPinv of the tall rank-deficient problem (or of its transpose), factored once per case and shared"""
    key = (shape, dtype, wide)
    if key not in _OPS:
        F = problem_def(*shape, NP[dtype])[0]
        _OPS[key] = lo.opPinv(dev_matrix(F.T, dtype, dev) if wide else dev_matrix(F, dtype, dev, LD.get(shape)))
    return _OPS[key]


def apply(lo, w, x, dtype, dev):
    return q.apply(lo, w, x, dtype, dev)


# ------------------------------------------------------------------------------------------------ 1. rank, permutation, storage
def check_factor(op, shape, dtype):
    mf, nf, r = shape
    eps = float(torch.finfo(dtype).eps)
    nblk = -(-r // 64)
    assert isinstance(op._rank, int) and op._rank == r, (shape, op._rank)
    perm = op._perm
    assert perm.dtype is torch.int32 and perm.is_cuda and tuple(perm.shape) == (nf,)
    assert sorted(perm.cpu().tolist()) == list(range(nf))
    assert op._rtol == max(mf, nf) * eps
    assert len(op._factor) == (8 if r < nf else 5) and op._factor[4] is perm
    W = op._factor[0]
    assert tuple(W.shape) == (mf, nf) and op._deps == (W,)
    if r < nf:
        W2, T2, D2 = op._factor[5:]
        assert tuple(W2.shape) == (nf, r) and W2.stride() == (1, nf) and W2.dtype is dtype
        assert T2.dtype is torch.float64 and T2.numel() == nblk * 64 * 64 and D2.dtype is torch.float64 and D2.numel() == nblk * 64 * 64
        # R2' R2 = S' S = [R11 R12] [R11 R12]': the second factor is the QR factor of the leading r rows of R
        R = np.triu(host(W[:nf, :]))[:r, :]
        R2 = np.triu(host(W2[:r, :]))
        err = float(np.linalg.norm(R2.T @ R2 - R @ R.T, 2) / np.linalg.norm(R, 2) ** 2)
        held(f"second factor {shape} {dtype}", err, mf * eps)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rank_permutation_and_storage(lo, dev, shape, dtype):
    op = factored(lo, dev, shape, dtype)
    assert tuple(op.shape) == (shape[1], shape[0]) and op._tall
    check_factor(op, shape, dtype)
    wide = factored(lo, dev, shape, dtype, wide=True)
    assert tuple(wide.shape) == shape[:2] and wide._tall == (shape[0] == shape[1])
    check_factor(wide, shape, dtype)


# ------------------------------------------------------------------------------------------------ 2. the four metrics
def check_metrics(lo, dev, tag, shape, dtype, opx, opy):
    mf = shape[0]
    F, v, nF = problem_def(*shape, NP[dtype])
    u = rhs_u(*shape, NP[dtype])
    eps = float(torch.finfo(dtype).eps)
    x = apply(lo, opx, v, dtype, dev)
    y = apply(lo, opy, u, dtype, dev)
    names = ("lsq x", "lsq y", "row space x", "range y")
    for name, e in zip(names, four_metrics(F, nF, v, u, x, y)):
        held(f"{name} {tag} {shape} {dtype}", e, mf * eps)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_minimum_norm_least_squares_solutions(lo, dev, shape, dtype):
    """x = F⁺ v and y = (F⁺)' u through opPinv(F) and its transpose, and through opPinv(F') and its transpose"""
    tall = factored(lo, dev, shape, dtype)
    check_metrics(lo, dev, "opPinv(F)", shape, dtype, tall, lo.transpose(tall))
    wide = factored(lo, dev, shape, dtype, wide=True)
    check_metrics(lo, dev, "opPinv(F')", shape, dtype, lo.transpose(wide), wide)


@gpu
@pytest.mark.parametrize("wide", [False, True], ids=["tall", "wide"])
def test_row_major_storage(lo, dev, wide):
    shape, dtype = (129, 65, 64), torch.float64
    F = problem_def(*shape, np.float64)[0]
    Ad = dev_matrix(F.T if wide else F, dtype, dev, rowmajor=True)
    before = Ad.clone()
    op = lo.opPinv(Ad)
    check_factor(op, shape, dtype)
    if wide:
        check_metrics(lo, dev, "row-major F'", shape, dtype, lo.transpose(op), op)
    else:
        check_metrics(lo, dev, "row-major F", shape, dtype, op, lo.transpose(op))
    assert torch.equal(Ad, before)


# ------------------------------------------------------------------------------------------------ 3. shorter than the basic solution
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_shorter_than_the_basic_solution(lo, dev, shape, dtype):
    mf, nf, r = shape
    assert r < nf
    F, v, nF = problem_def(*shape, NP[dtype])
    eps = float(torch.finfo(dtype).eps)
    x = apply(lo, factored(lo, dev, shape, dtype), v, dtype, dev)
    xb = apply(lo, lo.opQR(dev_matrix(F, dtype, dev, LD.get(shape)), pivot=True), v, dtype, dev)
    held(f"lsq pinv {shape} {dtype}", lsq_error(F, nF, v, x), mf * eps)
    held(f"lsq basic {shape} {dtype}", lsq_error(F, nF, v, xb), mf * eps)
    print(f"norms {shape} {dtype}: basic / minimum-norm = {np.linalg.norm(xb) / np.linalg.norm(x):.4f}")
    assert np.linalg.norm(x) < np.linalg.norm(xb)


# ------------------------------------------------------------------------------------------------ 4. the two modes are adjoint
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_two_modes_are_adjoint(lo, dev, shape, dtype):
    """|u' (F⁺ v) - v' ((F⁺)' u)| <= mf eps |F⁺| |u| |v|, and |F⁺| = 1: the smallest non-zero singular value of F is 1"""
    mf = shape[0]
    F, v, _ = problem_def(*shape, NP[dtype])
    u = rhs_u(*shape, NP[dtype])
    eps = float(torch.finfo(dtype).eps)
    op = factored(lo, dev, shape, dtype)
    x = apply(lo, op, v, dtype, dev)
    y = apply(lo, lo.transpose(op), u, dtype, dev)
    held(f"adjoint {shape} {dtype}", abs(float(u @ x - v @ y)), mf * eps * 1.0 * float(np.linalg.norm(u) * np.linalg.norm(v)))


# ------------------------------------------------------------------------------------------------ 5. Penrose conditions
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_penrose_conditions(lo, dev, dtype):
    """X = to_dense(opPinv(F)), through the block form. Each column of X is a backward-stable solve, X = (F + dF)⁺ with |dF| <=
    mf eps |F| (a different dF per column; the constants are dropped as everywhere in these files). With G = F + dF and G X G = G,
    X G X = X, G X and X G symmetric projectors of norm 1, to first order
        F X F - F = dF - dF X G - G X dF        -> mf eps |F|          scale |F|
        X F X - X = -X dF X                     -> mf eps |F| |X| |X|  scale |X|, with cond = |F| |X|
        (F X)' - F X = (dF X) - (dF X)'         -> mf eps |F| |X|      scale |F X| = 1
        (X F)' - X F = (X dF) - (X dF)'         -> mf eps |F| |X|      scale |X F| = 1
    so each is held to mf eps cond times the 2-norm of the matrix its condition names — F, X, F X, X F — with cond = 2, the
    singular values of F being 1 .. 2."""
    shape = (200, 129, 65)
    mf, nf, r = shape
    F = problem_def(*shape, NP[dtype])[0]
    eps = float(torch.finfo(dtype).eps)
    X = host(lo.to_dense(factored(lo, dev, shape, dtype)))
    assert X.shape == (nf, mf) and np.isfinite(X).all()
    cond, n2 = 2.0, lambda M: float(np.linalg.norm(M, 2))
    FX, XF = F @ X, X @ F
    held(f"penrose F X F = F {dtype}", n2(FX @ F - F), mf * eps * cond * n2(F))
    held(f"penrose X F X = X {dtype}", n2(XF @ X - X), mf * eps * cond * n2(X))
    held(f"penrose (F X)' = F X {dtype}", n2(FX.T - FX), mf * eps * cond * n2(FX))
    held(f"penrose (X F)' = X F {dtype}", n2(XF.T - XF), mf * eps * cond * n2(XF))


# ------------------------------------------------------------------------------------------------ 6. full rank
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("shape", [(200, 129), (64, 64)], ids=["200x129", "64x64"])
def test_full_rank_is_the_pivoted_operator_bit_for_bit(lo, dev, shape, dtype):
    m, n = shape
    A, v, u, _ = q.problem(m, n, NP[dtype])
    Ad = dev_matrix(A, dtype, dev)
    op, ref = lo.opPinv(Ad), lo.opQR(Ad, pivot=True)
    assert op._rank == n == ref._rank and len(op._factor) == 5
    assert torch.equal(op._perm, ref._perm) and torch.equal(op._factor[0], ref._factor[0])
    for w, wr, x, nres in ((op, ref, v, n), (lo.transpose(op), lo.transpose(ref), u, m)):
        xd = dev_vec(x, dtype, dev)
        res = torch.full((nres,), float("nan"), dtype=dtype, device=dev)
        want = torch.full((nres,), float("nan"), dtype=dtype, device=dev)
        torch.cuda.synchronize()
        a = counters(lo)
        lo.mul(res, w, xd)
        b = counters(lo)
        lo.mul(want, wr, xd)
        assert b["launch"] - a["launch"] == lo.linalg.qrp_launches(n) == lo.linalg.pinv_launches(n, n)
        assert torch.equal(res, want)


# ------------------------------------------------------------------------------------------------ 7. contract of the hot path
@gpu
@pytest.mark.parametrize("shape", [(200, 129, 65), (129, 65, 64)], ids=["200x129r65", "129x65r64"])
def test_an_apply_is_reproducible_capturable_and_only_launches(lo, dev, shape):
    dtype = torch.float64
    mf, nf, r = shape
    v = problem_def(*shape, np.float64)[1]
    u = rhs_u(*shape, np.float64)
    op = factored(lo, dev, shape, dtype)
    for w, x, nres in ((op, v, nf), (lo.transpose(op), u, mf)):
        xd = dev_vec(x, dtype, dev)
        res0 = torch.linspace(-1, 1, nres, dtype=dtype, device=dev)
        plain = torch.full((nres,), float("nan"), dtype=dtype, device=dev)
        lo.mul(plain, w, xd)                                              # beta == 0: the NaN of res is not read
        assert np.isfinite(host(plain)).all()
        runs = []
        for _ in range(2):
            res = res0.clone()
            lo.mul(res, w, xd, 2.0, -0.5)
            runs.append(res)
        assert torch.equal(runs[0], runs[1])
        want = 2.0 * host(plain) - 0.5 * host(res0)
        eps = np.finfo(np.float64).eps
        err = np.abs(host(runs[0]) - want)
        lim = 2 * eps * (2.0 * np.abs(host(plain)) + 0.5 * np.abs(host(res0)))
        print(f"alpha beta {shape}: max {float(np.max(err - lim)):.3e} over the 2 eps allowance")
        assert (err <= lim).all()
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
        d = {key: b[key] - a[key] for key in q.NAMES}
        assert d["launch"] == lo.linalg.pinv_launches(r, nf) == 3 * -(-r // 64) + 2, d
        assert not {key: x for key, x in d.items() if key != "launch" and x}, d


# ------------------------------------------------------------------------------------------------ 8. block form
@gpu
@pytest.mark.parametrize("wide", [False, True], ids=["tall", "wide"])
def test_a_matrix_operand_equals_its_columns_bit_for_bit(lo, dev, wide):
    dtype, shape = torch.float64, (200, 129, 65)
    mf, nf, r = shape
    base = factored(lo, dev, shape, dtype, wide=wide)
    rng = np.random.default_rng(13)
    for w in (base, lo.transpose(base)):
        nout, nin = lo.size(w, 1), lo.size(w, 2)
        for k in (1, 7, 8, 9, 17):
            V = torch.from_numpy(rng.standard_normal((k, nin))).to(dtype).to(dev).t()      # column-major nin x k
            R0 = torch.from_numpy(rng.standard_normal((k, nout))).to(dtype).to(dev).t()
            R = R0.clone(memory_format=torch.preserve_format)
            torch.cuda.synchronize()
            a = counters(lo)
            lo.mul(R, w, V, 2.0, -0.5)
            b = counters(lo)
            assert b["launch"] - a["launch"] == lo.linalg.pinv_block_launches(r, nf, k), (k, b["launch"] - a["launch"])
            for j in range(k):
                x = R0[:, j].clone()
                lo.mul(x, w, V[:, j].clone(), 2.0, -0.5)
                assert torch.equal(R[:, j], x), (k, j)


# ------------------------------------------------------------------------------------------------ 9. res may be v
@gpu
def test_res_may_be_v_for_a_square_operator(lo, dev):
    shape, dtype = (64, 64, 32), torch.float64
    op = factored(lo, dev, shape, dtype)
    v = problem_def(*shape, np.float64)[1]
    for w in (op, lo.transpose(op)):
        out = dev_vec(np.zeros(64), dtype, dev)
        lo.mul(out, w, dev_vec(v, dtype, dev), 2.0, 0.0)
        xv = dev_vec(v, dtype, dev)
        lo.mul(xv, w, xv, 2.0, 0.0)
        assert torch.equal(xv, out)
        out = dev_vec(v, dtype, dev)                                      # beta != 0: res = v is read as res as well
        tmp = dev_vec(v, dtype, dev)
        lo.mul(out, w, tmp, 2.0, -0.5)
        xv = dev_vec(v, dtype, dev)
        lo.mul(xv, w, xv, 2.0, -0.5)
        assert torch.equal(xv, out)


# ------------------------------------------------------------------------------------------------ 10. rtol
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_rtol_moves_the_rank_cut(lo, dev, dtype):
    """rtol = 0.9 cuts inside the non-zero singular values: the operator is then the pseudo-inverse of the TRUNCATED matrix
    Q1[:, 0:r'] [R11 R12] P', whose row space is P range([R11 R12]'), read here from the operator's own W and perm"""
    shape = (200, 129, 65)
    mf, nf, _ = shape
    F, v, _ = problem_def(*shape, NP[dtype])
    eps = float(torch.finfo(dtype).eps)
    Ad = dev_matrix(F, dtype, dev)
    full = lo.opPinv(Ad, rtol=0.0)
    assert full._rank == 129 and len(full._factor) == 5 and full._rtol == 0.0
    d = np.abs(np.diag(host(factored(lo, dev, shape, dtype)._factor[0][:129, :])))
    mid = float(np.sqrt(d[64] * d[65]) / d[0])                            # between the two sides of the gap
    assert d[65] / d[0] < mid < d[64] / d[0] and mid > 200 * eps
    op = lo.opPinv(Ad, rtol=mid)
    assert op._rank == 65 and op._rtol == mid and len(op._factor) == 8
    op = lo.opPinv(Ad, rtol=0.9)
    rt = op._rank
    assert 1 <= rt < 65 and op._rtol == 0.9 and tuple(op._factor[5].shape) == (nf, rt)
    x = apply(lo, op, v, dtype, dev)
    perm = op._perm.cpu().numpy()
    S = np.triu(host(op._factor[0][:nf, :]))[:rt, :].T                   # [R11 R12]' of the truncated factorisation, nf x r'
    B = np.linalg.qr(S)[0]
    y = x[perm]
    held(f"row space of the truncated matrix, rank {rt}, {dtype}", float(np.linalg.norm(y - B @ (B.T @ y)) / np.linalg.norm(y)), mf * eps)


# ------------------------------------------------------------------------------------------------ 11. exceptions
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_only_a_zero_matrix_or_a_non_finite_norm_raises(lo, dev, dtype):
    with pytest.raises(lo.SingularException) as ei:
        lo.opPinv(dev_matrix(np.zeros((70, 40)), dtype, dev))
    assert ei.value.info == 1
    A = np.array(q.problem(137, 84, NP[dtype])[0])
    B = A.copy()
    B[50, 30] = np.nan
    with pytest.raises(lo.SingularException) as ei:
        lo.opPinv(dev_matrix(B, dtype, dev))
    assert 1 <= ei.value.info <= 84
    A[:, 70] = 0.0
    A[:, 3] = 0.0
    op = lo.opPinv(dev_matrix(A, dtype, dev))
    assert op._rank == 82 and sorted(op._perm[82:].cpu().tolist()) == [3, 70]
    v = q.problem(137, 84, NP[dtype])[1]
    x = apply(lo, op, v, dtype, dev)
    held(f"zero columns {dtype}", float(np.max(np.abs(x[[3, 70]])) / np.linalg.norm(x)), 137 * float(torch.finfo(dtype).eps))
