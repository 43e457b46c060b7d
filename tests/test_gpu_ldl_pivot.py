"""opLDL(M, pivot=True) on the device (csrc/linalg.hip: mxlo_sytrf, mxlo_ldlp_mul, mxlo_ldlp_mul_block) against NumPy and torch's CPU
LAPACK in Float64 on the host. The matrices, the sizes and the bound eta <= 3 n eps(T) are those of ldl_pivot_cases.py, which
test_ldl_pivot_host.py holds LAPACK itself against."""
import ctypes as C

import numpy as np
import pytest
import torch

import ldl_pivot_cases as pc

gpu = pytest.mark.gpu
NB = pc.NB
NAMES = ("malloc", "free", "h2d", "d2h", "d2d", "d2h_bytes", "stream_sync", "device_sync", "event_sync", "memset_async",
         "launch", "blocking_copy")
COMBOS = pc.combos()
IDS = [f"{c}-{n}" for c, n in COMBOS]


def dev_matrix(A, dtype, dev, ld=None, rowmajor=False):
    """A on the device: column-major in a leading dimension ld >= n (the padding holds NaN), or row-major."""
    n = A.shape[0]
    t = torch.from_numpy(np.array(A)).to(dtype).to(dev)
    if rowmajor:
        return t.contiguous()
    ld = ld or max(n, 1)
    buf = torch.full((ld * A.shape[1],), float("nan"), dtype=dtype, device=dev)
    out = buf.as_strided(A.shape, (1, ld))
    out.copy_(t)
    return out


def dev_vec(x, dtype, dev):
    return torch.from_numpy(np.array(x)).to(dtype).to(dev)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def check_eta(tag, M, nM, x, v, n, dtype):
    assert np.isfinite(x).all(), tag
    e = pc.eta(M, nM, x, v)
    b = pc.bound(n, dtype)
    print(f"eta {tag}: {e:.3e} = {e / b * 3:.3f} n eps")
    assert e <= b, (tag, e / b)                             # 3 n eps(T): derived (ldl_pivot_cases.py)


def solve_and_check(lo, dev, case, n, dtype, rowmajor=False):
    M, v, nM, _ = pc.problem(case, n, pc.NP[dtype])
    Ml = M
    if rowmajor:
        Ml = M.copy()
        Ml[np.tril_indices(n, -1)] = np.nan                 # only the upper triangle may be read
    Md = dev_matrix(Ml, dtype, dev, pc.LD.get(n), rowmajor)
    before = Md.clone()
    op = lo.opLDL(Md, pivot=True)
    assert torch.equal(torch.nan_to_num(Md), torch.nan_to_num(before))       # M is not modified
    assert op.symmetric and op.hermitian and op.size() == (n, n) and op.eltype is dtype
    vd = dev_vec(v, dtype, dev)
    for name, w in (("op", op), ("transpose", lo.transpose(op)), ("adjoint", lo.adjoint(op))):
        res = torch.full((n,), float("nan"), dtype=dtype, device=dev)       # beta == 0: res is not read
        lo.mul(res, w, vd)
        check_eta(f"{case} {name} n={n} {dtype}", M, nM, host(res), v, n, dtype)
    return op


# ------------------------------------------------------------------------------------------------ 1. backward error
@gpu
@pytest.mark.parametrize("dtype", pc.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case,n", COMBOS, ids=IDS)
def test_backward_error_of_the_solve_and_of_its_transpose_and_adjoint(lo, dev, case, n, dtype):
    solve_and_check(lo, dev, case, n, dtype)


@gpu
@pytest.mark.parametrize("case", ["indef", "pairs1"])
def test_backward_error_over_seventeen_panels(lo, dev, case):
    solve_and_check(lo, dev, case, pc.N_BIG, torch.float64)


@gpu
@pytest.mark.parametrize("dtype", pc.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", pc.CASES)
def test_row_major_matrices_are_read_in_place(lo, dev, case, dtype):
    solve_and_check(lo, dev, case, 129, dtype, rowmajor=True)


# ------------------------------------------------------------------------------------------------ 2. unpivoted versus pivoted
@gpu
@pytest.mark.parametrize("dtype", pc.DTYPES, ids=["f64", "f32"])
def test_the_unpivoted_factorisation_raises_where_the_pivoted_one_solves(lo, dev, dtype):
    J = np.array([[0.0, 1.0], [1.0, 0.0]])
    with pytest.raises(lo.ZeroPivotException) as z:
        lo.opLDL(dev_matrix(J, dtype, dev))
    assert z.value.info == 1
    op = lo.opLDL(dev_matrix(J, dtype, dev), pivot=True)
    x = host(lo.apply(op, dev_vec(np.array([3.0, -5.0]), dtype, dev)))
    assert np.array_equal(x, [-5.0, 3.0])
    assert lo.ldl_inertia(op) == (1, 1, 0)
    for n in (2, 65, 130):
        M, v, nM, _ = pc.problem("saddle0", n, pc.NP[dtype])
        with pytest.raises(lo.ZeroPivotException) as z:
            lo.opLDL(dev_matrix(M, dtype, dev))
        assert z.value.info == 1
        op = lo.opLDL(dev_matrix(M, dtype, dev), pivot=True)
        check_eta(f"saddle0 n={n} {dtype}", M, nM, host(lo.apply(op, dev_vec(v, dtype, dev))), v, n, dtype)


# ------------------------------------------------------------------------------------------------ 3. the factor read back
def read_factor(op, n):
    W = host(op._factor[0])
    L = np.tril(W, -1) + np.eye(n)
    return L, host(op._d), host(op._e), op._perm.cpu().numpy().astype(np.int64)


@gpu
@pytest.mark.parametrize("dtype", pc.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case,n", COMBOS, ids=IDS)
def test_the_factor_reconstructs_the_permuted_matrix(lo, dev, case, n, dtype):
    """|L D L' - M[perm][:, perm]|_F <= 3 n eps |  |L| |D| |L'|  |_F: the componentwise bound of Higham Thm 11.3, normwise."""
    M = pc.problem(case, n, pc.NP[dtype])[0]
    op = lo.opLDL(dev_matrix(M, dtype, dev, pc.LD.get(n)), pivot=True)
    assert op._perm.dtype is torch.int32 and op._perm.shape == (n,) and op._perm.is_cuda
    for t in (op._d, op._e):
        assert t.dtype is torch.float64 and t.shape == (n,) and t.is_cuda
    L, d, e, perm = read_factor(op, n)
    assert sorted(perm.tolist()) == list(range(n))
    assert np.array_equal(np.diag(host(op._factor[0])), d)  # the diagonal of the storage is the diagonal of D
    two = np.nonzero(e)[0]
    assert e[n - 1] == 0.0 and not e[two + 1].any()         # e[k] != 0 => e[k + 1] == 0
    assert not L[two + 1, two].any()                        # unit lower: nothing below the diagonal inside a 2 x 2 block
    D = pc.block_diag_of(d, e)
    R = L @ D @ L.T - M[np.ix_(perm, perm)]
    rhs = np.abs(L) @ np.abs(D) @ np.abs(L).T
    r = np.linalg.norm(R) / np.linalg.norm(rhs)
    print(f"reconstruction {case} n={n} {dtype}: {r / pc.bound(n, dtype) * 3:.3f} n eps")
    assert r <= pc.bound(n, dtype)


@gpu
@pytest.mark.parametrize("n", pc.PIVOT_NS)
def test_the_pivots_are_lapacks(lo, dev, n):
    """So that growth cannot hide in the right-hand side of the reconstruction bound: the permutation and the 2 x 2 positions
    equal sytrf's (and the NumPy model's). These matrices have no ties; a comparison that flips under another summation
    order has probability of the order of eps."""
    M = pc.problem("indef", n, np.float64)[0]
    op = lo.opLDL(dev_matrix(M, torch.float64, dev), pivot=True)
    _, d, e, perm = read_factor(op, n)
    lperm, ltwo = pc.lapack_pivots(M)
    assert np.array_equal(perm, lperm)
    assert set(np.nonzero(e)[0].tolist()) == ltwo
    mperm, _, md, me = pc.bunch_kaufman(M)
    assert np.array_equal(perm, mperm) and np.array_equal(e != 0, me != 0)


# ------------------------------------------------------------------------------------------------ 4. inertia
@gpu
@pytest.mark.parametrize("case,n", COMBOS, ids=IDS)
def test_the_inertia_is_the_sign_count_of_the_eigenvalues(lo, dev, case, n):
    M, _, _, w = pc.problem(case, n, np.float64)
    op = lo.opLDL(dev_matrix(M, torch.float64, dev), pivot=True)
    assert lo.ldl_inertia(op) == (int((w > 0).sum()), int((w < 0).sum()), 0)
    d, e = host(op._d), host(op._e)
    for k in np.nonzero(e)[0]:
        assert d[k] * d[k + 1] - e[k] * e[k] < 0            # a 2 x 2 block Bunch-Kaufman chose is indefinite


@gpu
def test_the_inertia_of_an_unpivoted_operator(lo, dev):
    M = np.diag([2.0, -1.0, 3.0, -4.0, 5.0])
    assert lo.ldl_inertia(lo.opLDL(dev_matrix(M, torch.float64, dev))) == (3, 2, 0)


# ------------------------------------------------------------------------------------------------ 5. exceptions
def healthy_apply(lo, dev, dtype):
    n = 65
    M, v, nM, _ = pc.problem("indef", n, pc.NP[dtype])
    op = lo.opLDL(dev_matrix(M, dtype, dev), pivot=True)
    check_eta(f"healthy n={n} {dtype}", M, nM, host(lo.apply(op, dev_vec(v, dtype, dev))), v, n, dtype)


@gpu
@pytest.mark.parametrize("dtype", pc.DTYPES, ids=["f64", "f32"])
def test_unusable_pivots_raise_with_the_index_of_their_step(lo, dev, dtype):
    n = 65
    singular = np.eye(n)
    singular[63:, 63:] = 1.0                                # blockdiag(I_63, [[1, 1], [1, 1]]): the Schur complement at step 65 is 1 - 1
    nan00 = pc.problem("indef", n, pc.NP[dtype])[0].copy()
    nan00[0, 0] = np.nan
    nan_late = pc.problem("indef", 130, pc.NP[dtype])[0].copy()
    nan_late[129, 100] = nan_late[100, 129] = np.nan
    for name, M, info in (("zero", np.zeros((5, 5)), 1), ("diag(1, 0, 1)", np.diag([1.0, 0.0, 1.0]), 2), ("NaN at (0, 0)", nan00, 1),
                          ("singular at the panel end", singular, 65)):
        with pytest.raises(lo.ZeroPivotException) as z:
            lo.opLDL(dev_matrix(M, dtype, dev), pivot=True)
        assert z.value.info == info, name
        healthy_apply(lo, dev, dtype)
    try:                                                    # a NaN anywhere: the exception or a non-finite result, never a fault
        op = lo.opLDL(dev_matrix(nan_late, dtype, dev), pivot=True)
        x = host(lo.apply(op, dev_vec(np.ones(130), dtype, dev)))
        assert not np.isfinite(x).all()
    except lo.ZeroPivotException as z:
        assert 1 <= z.info <= 130
    healthy_apply(lo, dev, dtype)


@gpu
def test_check_true_refuses_a_non_symmetric_matrix_first(lo, dev):
    A = np.triu(np.ones((5, 5)))
    with pytest.raises(lo.LinearOperatorException, match="not Hermitian"):
        lo.opLDL(dev_matrix(A, torch.float64, dev), check=True, pivot=True)
    M, v, nM, _ = pc.problem("saddle0", 5, np.float64)
    op = lo.opLDL(dev_matrix(M, torch.float64, dev), check=True, pivot=True)
    check_eta("check=True", M, nM, host(lo.apply(op, dev_vec(v, torch.float64, dev))), v, 5, torch.float64)


# ------------------------------------------------------------------------------------------------ 6. the block form
@gpu
@pytest.mark.parametrize("dtype", pc.DTYPES, ids=["f64", "f32"])
def test_mul_on_a_matrix_equals_the_single_applies_bit_for_bit(lo, dev, dtype):
    n = 2 * NB + 2                                          # pairs1 at 130: a 2 x 2 pivot across both block boundaries
    op = lo.opLDL(dev_matrix(pc.problem("pairs1", n, pc.NP[dtype])[0], dtype, dev), pivot=True)
    rng = np.random.default_rng(8)
    for k in (1, 3, 8, 9):
        V = dev_matrix(rng.standard_normal((n, k)), dtype, dev, n + 3)       # a leading dimension > n, NaN in the padding
        R0 = dev_matrix(rng.standard_normal((n, k)), dtype, dev, n + 5)
        want = []
        for j in range(k):
            r = R0[:, j].clone()
            lo.mul(r, op, V[:, j].clone(), 2.0, -0.5)
            want.append(r)
        for w in (op, lo.transpose(op)):
            R = dev_matrix(host(R0), dtype, dev, n + 5)
            lo.mul(R, w, V, 2.0, -0.5)
            for j in range(k):
                assert torch.equal(R[:, j], want[j]), (k, j)
        X = dev_matrix(host(V), dtype, dev, n + 3)          # res is V
        lo.mul(X, op, X, 2.0, 0.0)
        for j in range(k):
            r = torch.full((n,), float("nan"), dtype=dtype, device=dev)
            lo.mul(r, op, V[:, j].clone(), 2.0, 0.0)
            assert torch.equal(X[:, j], r), (k, j)


@gpu
def test_res_is_v_and_partial_overlap_is_refused(lo, dev):
    n, dtype = NB + 1, torch.float64
    M, v, nM, _ = pc.problem("pairs1", n, np.float64)
    op = lo.opLDL(dev_matrix(M, dtype, dev), pivot=True)
    xv = dev_vec(v, dtype, dev)
    lo.mul(xv, op, xv, 1.0, 0.0)
    check_eta("res is v", M, nM, host(xv), v, n, dtype)
    buf = torch.ones(n + 1, dtype=dtype, device=dev)
    with pytest.raises(lo.MxloError, match="overlaps"):
        lo.mul(buf[1:], op, buf[:n], 1.0, 0.0)
    assert torch.equal(buf, torch.ones_like(buf))           # nothing was launched


# ------------------------------------------------------------------------------------------------ 7. contract of the hot path
def snap(lo):
    a = (C.c_int64 * 12)()
    lo._lib.call("mxlo_debug_counters", a)
    return dict(zip(NAMES, list(a)))


@gpu
@pytest.mark.parametrize("case", ["indef", "pairs1"])
def test_an_apply_is_reproducible_capturable_and_only_launches(lo, dev, case):
    import gc
    n, dtype = 4 * NB + 3, torch.float64
    M, v = pc.problem(case, n, np.float64)[:2]
    op = lo.opLDL(dev_matrix(M, dtype, dev), pivot=True)
    nblk = (n + NB - 1) // NB
    assert lo.ldlp_launches(n) <= 2 * nblk + 1
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
    assert d["launch"] == lo.ldlp_launches(n), d
    assert not {key: x for key, x in d.items() if key != "launch" and x}, d


# ------------------------------------------------------------------------------------------------ 8. inside a tree
@gpu
@pytest.mark.parametrize("dtype", pc.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", ["indef", "saddle0"])
def test_composition_returns_v_and_the_operator_is_symmetric(lo, dev, case, dtype):
    """opLDL(K, pivot=True) * LinearOperator(K): the product K v carries a relative error n eps, the solve has backward error
    3 n eps and turns a relative perturbation delta into cond(K) delta: |got - v| <= 3 n eps cond |v| with the constants
    dropped as everywhere. u'(op v) = v'(op u) for the exact inverse; each side is off by at most 3 n eps cond |K^-1| |u| |v|."""
    n = NB + 1
    K, v, nK, w = pc.problem(case, n, pc.NP[dtype])
    cond = nK / float(np.abs(w).min())
    eps = float(torch.finfo(dtype).eps)
    Kd = dev_matrix(K, dtype, dev)
    op = lo.opLDL(Kd, pivot=True)
    vd = dev_vec(v, dtype, dev)
    got = host(lo.apply(op * lo.LinearOperatorFromMatrix(Kd), vd))
    assert np.linalg.norm(got - v) <= 3 * n * eps * cond * np.linalg.norm(v)
    u = np.random.default_rng(11).standard_normal(n).astype(pc.NP[dtype]).astype(np.float64)
    ov, ou = host(lo.apply(op, vd)), host(lo.apply(op, dev_vec(u, dtype, dev)))
    tol = 3 * n * eps * cond * np.linalg.norm(u) * np.linalg.norm(v) / float(np.abs(w).min())
    assert abs(u @ ov - v @ ou) <= tol
