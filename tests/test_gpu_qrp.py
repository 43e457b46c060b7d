"""opQR(A, pivot=True) on the device (csrc/linalg.hip, linearoperators.jl_amd/linalg.py): the column-pivoted, rank-revealing QR
and the basic solutions through it, against numpy / LAPACK in Float64 on the host. The oracle has no rectangular solve.

Matrices. deficient(rng, m, n, r) = U diag(1 + i/(r-1)) V' with U (m x r) and V (n x r) from QR of Gaussians of
default_rng(9100 + 7 m + n): rank r exactly, the non-zero singular values in 1 .. 2. A is rounded to the device precision before
anything else is computed, so its numerical rank is r with singular values r + 1 .. of the order of eps |A|.

Shapes (mf, nf, r), the smallest at which block columns (NB = 64), row chunks and the rank cut can go wrong: see SHAPES.
(129, 65, 64) cuts exactly on a block edge, (200, 129, 65) one past it; (77, 40, 17) lives in a leading dimension of 79 with NaN in
the padding; (40001, 5, 3) has more row chunks than the 64 row groups a step of the factorisation may use.

Margins (test_the_inputs_sit_far_from_the_rank_threshold, CPU, LAPACK's geqp3 through scipy, default rtol = max(mf, nf) eps):
|R_rr| / (rtol |R_11|) >= 175 and |R_{r+1,r+1}| / (rtol |R_11|) <= 0.046 at every shape in both precisions, so a correct device
factorisation has a factor of more than 20 to spare on either side of the threshold.

Bounds. mf eps(T), the bound and the derivation of test_gpu_qr.py (Higham, Thms 19.4 and 20.3 with the constants and the
factor n dropped). Derived, not measured; LAPACK's basic solution stays at or below 0.18 of it at every shape here. Every test
prints observed / bound; the maxima seen on an MI355X are in DESIGN.md §4."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
NB = 64
SHAPES = [(5, 3, 2), (65, 64, 63), (65, 65, 1), (64, 64, 32), (129, 65, 64), (200, 129, 65), (300, 193, 128), (2049, 129, 100),
          (77, 40, 17), (40001, 5, 3)]
LD = {(77, 40, 17): 79}
IDS = [f"{m}x{n}r{r}" for m, n, r in SHAPES]
DTYPES = [torch.float64, torch.float32]
DIDS = ["f64", "f32"]
NP = {torch.float64: np.float64, torch.float32: np.float32}
NAMES = ("malloc", "free", "h2d", "d2h", "d2d", "d2h_bytes", "stream_sync", "device_sync", "event_sync", "memset_async",
         "launch", "blocking_copy")
# test 4: the range distance of LAPACK's own basic solution at (5, 3, 2) in Float64 is 0.91 of the bound with the seed of the
# shape (the bound is 5 eps there); the first seed offset at which it is at or below 0.25 — found on the host with scipy's
# geqp3: offsets 1 .. 8 give 0.29 .. 0.95, offset 9 gives 0.21 — is used for that case only
W_SEED_OFFSET = {((5, 3, 2), np.float64): 9}


def deficient(rng, m, n, r):
    U = np.linalg.qr(rng.standard_normal((m, r)))[0]
    V = np.linalg.qr(rng.standard_normal((n, r)))[0]
    return U @ np.diag(1 + np.arange(r) / max(r - 1, 1)) @ V.T


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def problem_def(m, n, r, npd):
    """(F, v, |F|_2) for the tall m x n matrix of rank r in the precision the device gets, as read-only Float64 arrays"""
    rng = np.random.default_rng(9100 + 7 * m + n)
    F = deficient(rng, m, n, r).astype(npd).astype(np.float64)
    v = rng.standard_normal(m).astype(npd).astype(np.float64)
    frozen(F, v)
    return F, v, float(np.linalg.norm(F, 2))


@functools.lru_cache(maxsize=None)
def consistent_rhs(m, n, r, npd):
    """u = F' w, rounded: a consistent right-hand side of the wide system F' y = u"""
    F = problem_def(m, n, r, npd)[0]
    rng = np.random.default_rng(9100 + 7 * m + n)
    off = W_SEED_OFFSET.get(((m, n, r), npd), 0)
    if off:
        rng = np.random.default_rng(9100 + 7 * m + n + off)               # the tuned case: w is the first draw of this seed
    else:
        deficient(rng, m, n, r)                                           # w is the draw after F and v
        rng.standard_normal(m)
    u = (F.T @ rng.standard_normal(m)).astype(npd).astype(np.float64)
    return frozen(u)[0]


def simple_matrix(rng, m, n):
    """test_gpu_qr.py's: U S V' with singular values 1 .. 2"""
    U = np.linalg.qr(rng.standard_normal((m, n)))[0]
    V = np.linalg.qr(rng.standard_normal((n, n)))[0]
    return U @ np.diag(1 + np.arange(n) / max(n - 1, 1)) @ V.T


@functools.lru_cache(maxsize=None)
def problem(m, n, npd):
    """test_gpu_qr.py's full-rank problem: (A, v, u, |A|_2)"""
    rng = np.random.default_rng(7300 + 7 * m + n)
    A = simple_matrix(rng, m, n).astype(npd).astype(np.float64)
    v = rng.standard_normal(m).astype(npd).astype(np.float64)
    u = rng.standard_normal(n).astype(npd).astype(np.float64)
    frozen(A, v, u)
    return A, v, u, float(np.linalg.norm(A, 2))


DELTA = {np.float64: 1e-6, np.float32: 1e-2}
NEAR = [(65, 64, 33), (200, 129, 65), (2049, 129, 100)]


@functools.lru_cache(maxsize=None)
def problem_near(m, n, r, npd):
    """every column is the unit vector u0 plus a perturbation of size delta out of a space of dimension r - 1: rank r, and
    after the first step the norms of all remaining columns have lost log10(1/delta) digits — what a downdated norm gets wrong"""
    rng = np.random.default_rng(9500 + 7 * m + n)
    u0 = rng.standard_normal(m)
    u0 /= np.linalg.norm(u0)
    F = np.outer(u0, np.ones(n)) + DELTA[npd] * np.sqrt(n) * deficient(rng, m, n, r - 1)
    F = F.astype(npd).astype(np.float64)
    v = rng.standard_normal(m).astype(npd).astype(np.float64)
    frozen(F, v)
    return F, v, float(np.linalg.norm(F, 2))


def dev_matrix(A, dtype, dev, ld=None, rowmajor=False):
    """A on the device: column-major in a leading dimension ld >= rows (the padding holds NaN), or row-major"""
    t = torch.from_numpy(np.array(A, order="C")).to(dtype).to(dev)
    if rowmajor:
        return t.contiguous()
    ld = ld or max(A.shape[0], 1)
    buf = torch.full((ld * A.shape[1],), float("nan"), dtype=dtype, device=dev)
    out = buf.as_strided(A.shape, (1, ld))
    out.copy_(t)
    return out


def dev_vec(x, dtype, dev):
    return torch.from_numpy(np.array(x)).to(dtype).to(dev)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


_OPS = {}


def factored(lo, dev, shape, dtype, wide=False):
    """opQR(., pivot=True) of the tall rank-deficient problem (or of its transpose), factored once per case and shared"""
    key = (shape, dtype, wide)
    if key not in _OPS:
        F = problem_def(*shape, NP[dtype])[0]
        _OPS[key] = lo.opQR(dev_matrix(F.T, dtype, dev) if wide else dev_matrix(F, dtype, dev, LD.get(shape)), pivot=True)
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


def wide_errors(F, nF, u, y):
    """(residual of F' y = u, distance of y from range(F)), both relative"""
    res = float(np.linalg.norm(F.T @ y - u) / (nF * np.linalg.norm(y) + np.linalg.norm(u)))
    Ur = range_basis(F.tobytes(), F.shape)
    return res, float(np.linalg.norm(y - Ur @ (Ur.T @ y)) / np.linalg.norm(y))


@functools.lru_cache(maxsize=None)
def range_basis(raw, shape):
    """an orthonormal basis of range(F): the left singular vectors above the gap (the others are of the order of eps |F|)"""
    U, sv, _ = np.linalg.svd(np.frombuffer(raw, dtype=np.float64).reshape(shape), full_matrices=False)
    return U[:, sv > 1e-3 * sv[0]]


def minimum_norm_errors(A, nA, u, y):
    """test_gpu_qr.py's two metrics for a full-rank A"""
    proj = A @ np.linalg.lstsq(A, y, rcond=None)[0]
    return float(np.linalg.norm(A.T @ y - u) / (nA * np.linalg.norm(y))), float(np.linalg.norm(y - proj) / np.linalg.norm(y))


def lapack_basic(F, npd, rtol=None):
    """(rank, |diag R|, perm, solve, solve_t) of LAPACK's geqp3 in the precision npd with this file's rank rule"""
    from scipy.linalg import qr, solve_triangular
    m, n = F.shape
    Q, R, perm = qr(F.astype(npd), mode="economic", pivoting=True)
    d = np.abs(np.diag(R)).astype(np.float64)
    rtol = max(m, n) * float(np.finfo(npd).eps) if rtol is None else rtol
    ok = d > rtol * d[0]
    r = int(n if ok.all() else np.argmin(ok))

    def solve(v):
        x = np.zeros(n, dtype=npd)
        x[perm[:r]] = solve_triangular(R[:r, :r], Q[:, :r].T @ v.astype(npd))
        return x.astype(np.float64)

    def solve_t(u):
        return (Q[:, :r] @ solve_triangular(R[:r, :r], u.astype(npd)[perm[:r]], trans="T")).astype(np.float64)

    return r, d, perm, solve, solve_t


# ------------------------------------------------------------------------------------------------ 0. the inputs (CPU)
@pytest.mark.parametrize("npd", [np.float64, np.float32], ids=DIDS)
def test_the_inputs_sit_far_from_the_rank_threshold(npd):
    """LAPACK's geqp3 on the matrices of this file: the rank comes out as r, with |R_rr| >= 175 and |R_{r+1,r+1}| <= 0.046 times
    the threshold rtol |R_11|; LAPACK's own basic solutions stay within 0.18 of the bounds (0.25 for the one tuned case)"""
    eps = float(np.finfo(npd).eps)
    worst = [np.inf, 0.0, 0.0, 0.0]
    cases = [(s, problem_def(*s, npd)) for s in SHAPES] + [(s, problem_near(*s, npd)) for s in NEAR]
    for k, (shape, (F, v, nF)) in enumerate(cases):
        m, n, r = shape
        rank, d, _, solve, solve_t = lapack_basic(F, npd)
        assert rank == r, (shape, rank)
        thr = max(m, n) * eps * d[0]
        worst[0] = min(worst[0], d[r - 1] / thr)
        if r < n:
            worst[1] = max(worst[1], d[r] / thr)
        worst[2] = max(worst[2], lsq_error(F, nF, v, solve(v)) / (m * eps))
        if k < len(SHAPES):
            e = wide_errors(F, nF, consistent_rhs(*shape, npd), solve_t(consistent_rhs(*shape, npd)))
            tuned = (shape, npd) in W_SEED_OFFSET
            assert max(e) / (m * eps) <= (0.25 if tuned else 0.18), (shape, e)
            worst[3] = max(worst[3], max(e) / (m * eps))
    print(f"margins {npd.__name__}: |R_rr| >= {worst[0]:.1f} thr, |R_r+1| <= {worst[1]:.3f} thr, lsq {worst[2]:.3f}, wide {worst[3]:.3f}")
    assert worst[0] >= 175 and worst[1] <= 0.046 and worst[2] <= 0.16


# ------------------------------------------------------------------------------------------------ 1. rank and permutation
def check_rank_perm(op, shape, dtype):
    mf, nf, r = shape
    eps = float(torch.finfo(dtype).eps)
    assert isinstance(op._rank, int) and op._rank == r, (shape, op._rank)
    perm = op._perm
    assert perm.dtype is torch.int32 and perm.is_cuda and tuple(perm.shape) == (nf,)
    assert sorted(perm.cpu().tolist()) == list(range(nf))
    assert op._factor[-1] is perm and op._rtol == max(mf, nf) * eps
    W = op._factor[0]
    assert tuple(W.shape) == (mf, nf)
    d = np.abs(np.diag(host(W[:nf, :])))[:r]
    assert np.isfinite(d).all()
    worst = float(np.max(d[1:] / d[:-1])) if r > 1 else 0.0
    print(f"rank {shape} {dtype}: max |R_j+1| / |R_j| = {worst:.6f}")
    assert worst <= 1 + mf * eps


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rank_and_permutation(lo, dev, shape, dtype):
    op = factored(lo, dev, shape, dtype)
    assert tuple(op.shape) == (shape[1], shape[0]) and op._tall
    check_rank_perm(op, shape, dtype)
    wide = factored(lo, dev, shape, dtype, wide=True)
    assert tuple(wide.shape) == shape[:2] and wide._tall == (shape[0] == shape[1])
    check_rank_perm(wide, shape, dtype)


@gpu
@pytest.mark.parametrize("wide", [False, True], ids=["tall", "wide"])
def test_row_major_storage(lo, dev, wide):
    shape, dtype = (129, 65, 64), torch.float64
    F, v, nF = problem_def(*shape, np.float64)
    Ad = dev_matrix(F.T if wide else F, dtype, dev, rowmajor=True)
    before = Ad.clone()
    op = lo.opQR(Ad, pivot=True)
    check_rank_perm(op, shape, dtype)
    x = apply(lo, lo.transpose(op) if wide else op, v, dtype, dev)
    held(f"lsq rowmajor wide={wide}", lsq_error(F, nF, v, x), shape[0] * np.finfo(np.float64).eps)
    assert torch.equal(Ad, before)


# ------------------------------------------------------------------------------------------------ 2. exact pivot order
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("shape", [(129, 65), (300, 193)], ids=["129x65", "300x193"])
def test_exact_pivot_order(lo, dev, shape, dtype):
    """orthonormal columns scaled by 1 + j/nf in a shuffled order: the norms of the remaining columns stay their scales, whose
    gaps 1/nf are far above eps, so the permutation is the descending order of the scales exactly"""
    m, n = shape
    rng = np.random.default_rng(9200 + 7 * m + n)
    Q = np.linalg.qr(rng.standard_normal((m, n)))[0]
    scales = 1 + rng.permutation(n) / n
    op = lo.opQR(dev_matrix(Q * scales, dtype, dev), pivot=True)
    assert op._rank == n
    assert op._perm.cpu().tolist() == np.argsort(-scales).tolist()


# ------------------------------------------------------------------------------------------------ 3. least squares
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_least_squares_of_a_rank_deficient_system(lo, dev, shape, dtype):
    """A square A' is its own tall orientation, so opQR(A') factors A' and its transposed mode is the basic solution of a
    CONSISTENT system with A, which a Gaussian v is not: the route through the transpose is taken for mf > nf only."""
    mf, nf, r = shape
    F, v, nF = problem_def(*shape, NP[dtype])
    eps = float(torch.finfo(dtype).eps)
    base = factored(lo, dev, shape, dtype)
    routes = [("op", base, base)]
    if mf > nf:
        wide = factored(lo, dev, shape, dtype, True)
        routes.append(("transpose(opQR(A'))", lo.transpose(wide), wide))
    for tag, op, owner in routes:
        perm = owner._perm.cpu().numpy()
        x = apply(lo, op, v, dtype, dev)
        held(f"lsq {tag} {shape} {dtype}", lsq_error(F, nF, v, x), mf * eps)
        zeros = np.flatnonzero(x == 0.0)
        assert sorted(zeros.tolist()) == sorted(perm[r:].tolist()), (tag, zeros, perm[r:])


# ------------------------------------------------------------------------------------------------ 4. consistent wide system
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_consistent_wide_system_of_a_rank_deficient_matrix(lo, dev, shape, dtype):
    """u = F' w is consistent, so the basic solution y solves F' y = u and lies in range(F). The right-hand side of (5, 3, 2) in
    Float64 comes from the seed offset W_SEED_OFFSET = 9, the first at which LAPACK's own range distance is at or below 0.25 of
    the bound (it is 0.91 at offset 0); no other input is tuned. A square A' is its own tall orientation: opQR(A') then solves
    A' y = u in the least-squares mode, whose basic solution has nf - r zeros and is a solution, but not the one in range(F)."""
    mf, nf, r = shape
    F, _, nF = problem_def(*shape, NP[dtype])
    u = consistent_rhs(*shape, NP[dtype])
    eps = float(torch.finfo(dtype).eps)
    for tag, w in (("transpose(op)", lo.transpose(factored(lo, dev, shape, dtype))), ("opQR(A')", factored(lo, dev, shape, dtype, True))):
        y = apply(lo, w, u, dtype, dev)
        res, dist = wide_errors(F, nF, u, y)
        held(f"wide residual {tag} {shape} {dtype}", res, mf * eps)
        if mf > nf or tag == "transpose(op)":
            held(f"wide range {tag} {shape} {dtype}", dist, mf * eps)


# ------------------------------------------------------------------------------------------------ 5. full rank
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("shape", [(65, 64), (200, 129), (2049, 129)], ids=["65x64", "200x129", "2049x129"])
def test_full_rank_matrices_are_solved_as_without_pivoting(lo, dev, shape, dtype):
    m, n = shape
    A, v, u, nA = problem(m, n, NP[dtype])
    eps = float(torch.finfo(dtype).eps)
    op = lo.opQR(dev_matrix(A, dtype, dev), pivot=True)
    assert op._rank == n
    held(f"full lsq {shape} {dtype}", lsq_error(A, nA, v, apply(lo, op, v, dtype, dev)), m * eps)
    res, dist = minimum_norm_errors(A, nA, u, apply(lo, lo.transpose(op), u, dtype, dev))
    held(f"full minnorm residual {shape} {dtype}", res, m * eps)
    held(f"full minnorm range {shape} {dtype}", dist, m * eps)


# ------------------------------------------------------------------------------------------------ 6. near-parallel columns
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("shape", NEAR, ids=[f"{m}x{n}r{r}" for m, n, r in NEAR])
def test_near_parallel_columns(lo, dev, shape, dtype):
    m, n, r = shape
    F, v, nF = problem_near(*shape, NP[dtype])
    eps = float(torch.finfo(dtype).eps)
    op = lo.opQR(dev_matrix(F, dtype, dev), pivot=True)
    assert op._rank == r, op._rank
    held(f"near-parallel lsq {shape} {dtype}", lsq_error(F, nF, v, apply(lo, op, v, dtype, dev)), m * eps)


# ------------------------------------------------------------------------------------------------ 7. rtol
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_rtol_moves_the_rank_cut(lo, dev, dtype):
    shape = (200, 129, 65)
    F, v, _ = problem_def(*shape, NP[dtype])
    eps = float(torch.finfo(dtype).eps)
    Ad = dev_matrix(F, dtype, dev)
    assert lo.opQR(Ad, pivot=True, rtol=0.0)._rank == 129
    d = np.abs(np.diag(host(factored(lo, dev, shape, dtype)._factor[0][:129, :])))
    mid = float(np.sqrt(d[64] * d[65]) / d[0])                            # between the two sides of the gap
    assert d[65] / d[0] < mid < d[64] / d[0] and mid > 200 * eps
    op = lo.opQR(Ad, pivot=True, rtol=mid)
    assert op._rank == 65 and op._rtol == mid
    op = lo.opQR(Ad, pivot=True, rtol=0.9)
    assert op._rank >= 1
    apply(lo, op, v, dtype, dev)                                          # asserts a finite result


# ------------------------------------------------------------------------------------------------ 8. exceptions
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_only_a_zero_matrix_or_a_non_finite_norm_raises(lo, dev, dtype):
    with pytest.raises(lo.SingularException) as ei:
        lo.opQR(dev_matrix(np.zeros((70, 40)), dtype, dev), pivot=True)
    assert ei.value.info == 1
    A = np.array(problem(137, 84, NP[dtype])[0])
    B = A.copy()
    B[50, 30] = np.nan
    with pytest.raises(lo.SingularException) as ei:
        lo.opQR(dev_matrix(B, dtype, dev), pivot=True)
    assert 1 <= ei.value.info <= 84
    A[:, 70] = 0.0
    op = lo.opQR(dev_matrix(A, dtype, dev), pivot=True)
    assert op._rank == 83 and int(op._perm[83]) == 70


# ------------------------------------------------------------------------------------------------ 9. contract of the hot path
def counters(lo):
    a = (C.c_int64 * 12)()
    lo._lib.call("mxlo_debug_counters", a)
    return dict(zip(NAMES, list(a)))


@gpu
@pytest.mark.parametrize("shape", [(200, 129, 65), (129, 65, 64)], ids=["200x129r65", "129x65r64"])
def test_an_apply_is_reproducible_capturable_and_only_launches(lo, dev, shape):
    import gc
    dtype = torch.float64
    mf, nf, r = shape
    F, v, _ = problem_def(*shape, np.float64)
    u = consistent_rhs(*shape, np.float64)
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
        d = {key: b[key] - a[key] for key in NAMES}
        assert d["launch"] == lo.linalg.qrp_launches(r), d
        assert d["launch"] <= lo.linalg.qr_launches(r) + 1
        assert not {key: x for key, x in d.items() if key != "launch" and x}, d


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


# ------------------------------------------------------------------------------------------------ 10. block form
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
            assert b["launch"] - a["launch"] == lo.linalg.qrp_block_launches(r, k), (k, b["launch"] - a["launch"])
            for j in range(k):
                x = R0[:, j].clone()
                lo.mul(x, w, V[:, j].clone(), 2.0, -0.5)
                assert torch.equal(R[:, j], x), (k, j)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_to_dense_is_a_left_inverse_on_the_pivot_columns(lo, dev, dtype):
    """X = to_dense(op) is the nf x mf matrix of the basic solve; F[:, perm[:r]] has full column rank and its columns are solved
    exactly by unit vectors, so (X F)[perm[:r], perm[:r]] = I to mf eps cond(F[:, perm[:r]])"""
    shape = (200, 129, 65)
    mf, nf, r = shape
    F = problem_def(*shape, NP[dtype])[0]
    eps = float(torch.finfo(dtype).eps)
    op = factored(lo, dev, shape, dtype)
    X = host(lo.to_dense(op))
    assert X.shape == (nf, mf)
    piv = op._perm.cpu().numpy()[:r]
    G = (X @ F[:, piv])[piv, :]
    held(f"to_dense {dtype}", float(np.linalg.norm(G - np.eye(r), 2)), mf * eps * float(np.linalg.cond(F[:, piv])))


# ------------------------------------------------------------------------------------------------ 11. pivot=False unchanged
@gpu
def test_pivot_false_is_the_unpivoted_operator(lo, dev):
    dtype, (m, n) = torch.float64, (200, 129)
    A, v, u, _ = problem(m, n, np.float64)
    Ad = dev_matrix(A, dtype, dev)
    ops = [lo.opQR(Ad), lo.opQR(Ad, pivot=False)]
    outs = []
    for op in ops:
        assert not hasattr(op, "_rank") and len(op._factor) == 4
        row = []
        for w, x, nres in ((op, v, n), (lo.transpose(op), u, m)):
            res = torch.full((nres,), float("nan"), dtype=dtype, device=dev)
            xd = dev_vec(x, dtype, dev)
            torch.cuda.synchronize()
            a = counters(lo)
            lo.mul(res, w, xd)
            b = counters(lo)
            assert b["launch"] - a["launch"] == lo.linalg.qr_launches(n)
            row.append(res)
        outs.append(row)
        assert torch.equal(op._factor[0], ops[0]._factor[0])
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
