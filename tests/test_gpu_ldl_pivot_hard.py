"""-m gpu: opLDL(M, pivot=True) (csrc/linalg.hip: mxlo_sytrf, mxlo_ldlp_mul, mxlo_ldlp_mul_block) on exact, tied, scaled and
non-finite inputs, and the contract of its block form. The cases and the rational model are tests/ldl_pivot_hard_cases.py;
tests/test_ldl_pivot_hard_host.py shows on the CPU that every exact factor is representable in Float32, that the rational
model, the NumPy model and LAPACK take the same pivots on them, and that LAPACK meets 3 n eps with a factor of two to spare.

Nothing here is a measured tolerance: the assertions are bit equality (with the rational model; between a block column and its
vector apply; between an operator and the operator of a power-of-two multiple of its matrix), the derived bound eta <= 3 n eps(T)
of ldl_pivot_cases.py, and the `info` of the NumPy model for a matrix with a non-finite entry.

a. the exact families: perm, d, e and the strict lower triangle of L equal the rational model's in both precisions
b. arrow_tie with more tied rows than the panel has threads: the first row wins through the stride loop
c. c M, c a power of two: the same pivots, the same bits of L, d and e scaled by c, the apply scaled by 1 / c
d. a NaN or +Inf in M raises ZeroPivotException with the model's info, wherever the entry is; the context stays usable
e. a NaN (Inf) in v leaves every entry of the result NaN (not finite); res is not read when beta == 0
f. the block form: non-finite columns stay in their column, padding and neighbours keep their bits, the launch count, and the
   refusals before any launch"""
import gc
import os
import re
import time

import numpy as np
import pytest
import torch

import ldl_pivot_cases as pc
import ldl_pivot_hard_cases as hc
import test_gpu_ldl_pivot as tp

pytestmark = pytest.mark.gpu
EXACT = hc.exact_cases()
IDS = [hc.case_id(*x) for x in EXACT]
DT_IDS = ["f64", "f32"]
ROW_MAJOR = [("arrow_tie", (130,)), ("gadget_sum", (130, 130)), ("saddle_pairs", (130, 0)), ("saddle_pairs", (130, 1)),
             ("perm_blocks", (130, 130))]
NAN = float("nan")


def bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def strict_lower(op):
    return np.tril(tp.host(op._factor[0]), -1)


def two_by_two(e):
    return set(np.nonzero(e)[0].tolist())


# ------------------------------------------------------------------------------------------------ a. exact factorisations
def check_against_the_model(lo, op, family, args, tag):
    perm, L, d, e, inertia = hc.exact_factor(family, args)
    n = len(d)
    _, dd, ed, permd = tp.read_factor(op, n)
    assert np.array_equal(permd, perm), (tag, "perm", np.nonzero(permd != perm)[0][:8].tolist())
    assert np.array_equal(dd, d), (tag, "d", np.nonzero(dd != d)[0][:8].tolist())
    assert np.array_equal(ed, e), (tag, "e", np.nonzero(ed != e)[0][:8].tolist())
    Ld = strict_lower(op)
    want = np.tril(L, -1)
    assert np.array_equal(Ld, want), (tag, "L", np.argwhere(Ld != want)[:8].tolist())
    assert np.array_equal(np.diag(tp.host(op._factor[0])), d), (tag, "the diagonal of the storage")
    assert lo.ldl_inertia(op) == inertia, tag
    return Ld, dd, ed, permd


@pytest.mark.parametrize("family,args", EXACT, ids=IDS)
def test_an_exact_factorisation_is_the_rational_model_bit_for_bit_in_both_precisions(lo, dev, family, args):
    M, nM, _ = hc.exact_matrix(family, args)
    n = M.shape[0]
    v = hc.exact_rhs(n)
    got = []
    for dtype in pc.DTYPES:
        tag = f"{hc.case_id(family, args)} {dtype}"
        op = lo.opLDL(tp.dev_matrix(M, dtype, dev), pivot=True)
        got.append(check_against_the_model(lo, op, family, args, tag))
        res = torch.full((n,), NAN, dtype=dtype, device=dev)
        lo.mul(res, op, tp.dev_vec(v, dtype, dev))
        tp.check_eta(tag, M, nM, tp.host(res), v, n, dtype)
    for a, b in zip(*got):                                  # Float32 widened is Float64
        assert np.array_equal(a, b)


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("family,args", ROW_MAJOR, ids=[hc.case_id(*x) for x in ROW_MAJOR])
def test_an_exact_factorisation_of_a_row_major_matrix_reads_one_triangle_only(lo, dev, family, args, dtype):
    M = hc.exact_matrix(family, args)[0].copy()
    M[np.tril_indices(M.shape[0], -1)] = np.nan             # only the upper triangle may be read
    op = lo.opLDL(tp.dev_matrix(M, dtype, dev, rowmajor=True), pivot=True)
    check_against_the_model(lo, op, family, args, f"row-major {hc.case_id(family, args)} {dtype}")


# ------------------------------------------------------------------------------------------------ b. the tie through the stride loop
def panel_threads(lo):
    src = os.path.join(os.path.dirname(os.path.abspath(lo.__file__)), "csrc", "linalg.hip")
    with open(src) as f:
        found = re.findall(r"constexpr int PT = (\d+);", f.read())
    assert len(found) == 1
    return int(found[0])


def test_a_tie_of_more_rows_than_the_panel_has_threads_goes_to_the_first_row(lo, dev):
    """Step 0 of arrow_tie(n): rows 1 .. n - 1 of column 0 all hold 1, every thread of the panel workgroup meets more than one of
    them in its stride loop, and row 1 has to win. The model's perm is 1, 2, .., n - 1, 0."""
    n = hc.stride_tie_n(panel_threads(lo))
    args = (n, hc.STRIDE_TIE_DIAG)
    perm, _, d, e, inertia = hc.exact_factor("arrow_tie", args)
    Md = tp.dev_matrix(hc.exact_matrix("arrow_tie", args)[0], torch.float64, dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    op = lo.opLDL(Md, pivot=True)
    torch.cuda.synchronize()
    print(f"arrow_tie n={n}: factorised in {time.perf_counter() - t0:.3f} s")
    permd = op._perm.cpu().numpy().astype(np.int64)
    assert permd[0] == 1, permd[:4]
    assert np.array_equal(permd, perm)
    assert np.array_equal(tp.host(op._d), d) and not tp.host(op._e).any() and not e.any()
    assert lo.ldl_inertia(op) == inertia == (n - 1, 1, 0)


# ------------------------------------------------------------------------------------------------ c. scaling by a power of two
@pytest.mark.parametrize("dtype", pc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", ["indef", "pairs1"])
def test_scaling_the_matrix_by_a_power_of_two_commutes_bit_for_bit(lo, dev, case, dtype):
    """Every comparison and every operation of the panel, the update and ldlp_dsolve_kernel is equivariant under a power of two
    as long as nothing over- or underflows; 2^+-40 (Float64) and 2^+-20 (Float32) keep every number far from both ends."""
    n = 130
    M, v = pc.problem(case, n, pc.NP[dtype])[:2]
    vd = tp.dev_vec(v, dtype, dev)
    op = lo.opLDL(tp.dev_matrix(M, dtype, dev), pivot=True)
    L, d, e, perm = strict_lower(op), tp.host(op._d), tp.host(op._e), op._perm.cpu().numpy()
    x = tp.host(lo.apply(op, vd))
    assert np.isfinite(x).all() and two_by_two(e)
    p = 40 if dtype is torch.float64 else 20
    for c in (2.0 ** p, 2.0 ** -p):
        ops = lo.opLDL(tp.dev_matrix(c * M, dtype, dev), pivot=True)
        assert np.array_equal(ops._perm.cpu().numpy(), perm), c
        assert two_by_two(tp.host(ops._e)) == two_by_two(e), c
        assert np.array_equal(strict_lower(ops), L), c
        assert np.array_equal(tp.host(ops._d), c * d) and np.array_equal(tp.host(ops._e), c * e), c
        assert np.array_equal(tp.host(lo.apply(ops, vd)), x / c), c


# ------------------------------------------------------------------------------------------------ d. non-finite entries of M
BAD_AT = [(0, 0), (63, 63), (64, 63), (64, 64), (65, 64), (129, 100), (129, 129), (100, 3)]


@pytest.mark.parametrize("value", [NAN, float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("dtype", pc.DTYPES, ids=DT_IDS)
def test_a_non_finite_entry_of_m_raises_with_the_index_of_the_step_that_meets_it(lo, dev, dtype, value):
    """The contract: a pivot that is zero or not finite raises with the index of its step. The NumPy model says which step that is;
    the entry reaches a column search or a diagonal by step max(i, j) + 1 at the latest."""
    n = 130
    base = pc.problem("indef", n, pc.NP[dtype])[0]
    for i, j in BAD_AT:
        M = base.copy()
        M[i, j] = M[j, i] = value
        with np.errstate(all="ignore"), pytest.raises(pc.ZeroPivot) as model:
            pc.bunch_kaufman(M)
        assert 1 <= model.value.info <= max(i, j) + 1
        with pytest.raises(lo.ZeroPivotException) as z:
            lo.opLDL(tp.dev_matrix(M, dtype, dev), pivot=True)
        print(f"{value} at ({i}, {j}) {dtype}: info {z.value.info}, model {model.value.info}")
        assert z.value.info == model.value.info, (i, j)
        tp.healthy_apply(lo, dev, dtype)


# ------------------------------------------------------------------------------------------------ e. non-finite entries of v
@pytest.mark.parametrize("dtype", pc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("case", ["indef", "pairs1"])
def test_a_non_finite_entry_of_v_reaches_every_entry_of_the_result(lo, dev, case, n, dtype):
    """L is dense and both sweeps multiply whole blocks of 64: wherever the entry is, the sweep with L' carries it to every row."""
    M, v = pc.problem(case, n, pc.NP[dtype])[:2]
    op = lo.opLDL(tp.dev_matrix(M, dtype, dev), pivot=True)
    for j in (0, 63, 64, n - 1):
        for value in (NAN, float("inf")):
            vp = v.copy()
            vp[j] = value
            for ab in ((), (2.0, 0.0)):
                res = torch.full((n,), NAN, dtype=dtype, device=dev)
                lo.mul(res, op, tp.dev_vec(vp, dtype, dev), *ab)
                x = tp.host(res)
                if np.isnan(value):
                    assert np.isnan(x).all(), (j, ab)
                else:
                    assert not np.isfinite(x).any(), (j, ab)
    res = torch.full((n,), NAN, dtype=dtype, device=dev)    # and a healthy v next to a NaN-filled res: beta == 0 does not read it
    lo.mul(res, op, tp.dev_vec(v, dtype, dev), 2.0, 0.0)
    assert np.isfinite(tp.host(res)).all()


# ------------------------------------------------------------------------------------------------ f. the block contract
BLOCK_NS = [63, 64, 65, 130]
BLOCK_KS = [2, 8, 9, 17]
OPS = {}


def operator(lo, dev, n, dtype=torch.float64):
    if (n, dtype) not in OPS:
        OPS[(n, dtype)] = lo.opLDL(tp.dev_matrix(pc.problem("pairs1", n, pc.NP[dtype])[0], dtype, dev), pivot=True)
    return OPS[(n, dtype)]


def operands(n, k):
    rng = np.random.default_rng(9300 + 31 * n + k)
    return rng.standard_normal((n, k)), rng.standard_normal((n, k))


def singles(lo, op, V, R0, a, b):
    out = []
    for j in range(V.shape[1]):
        r = R0[:, j].clone()
        lo.mul(r, op, V[:, j].clone(), a, b)
        out.append(r)
    return out


def abi_block(lo, dev, op, n, res, ldr, V, ldv, k, a=1.0, b=0.0):
    W, dinv, _, _, work = op._factor
    lo._lib.call("mxlo_ldlp_mul_block", lo.device.get_ctx(dev).handle, lo.device.dtype_code(op.eltype), res, ldr, W.data_ptr(), n, n,
                 dinv.data_ptr(), op._d.data_ptr(), op._e.data_ptr(), op._perm.data_ptr(), work.data_ptr(), V, ldv, k, a, b)


@pytest.mark.parametrize("k", BLOCK_KS)
@pytest.mark.parametrize("n", BLOCK_NS)
def test_a_nan_column_and_an_inf_column_stay_in_their_columns(lo, dev, n, k):
    dtype = torch.float64
    op = operator(lo, dev, n)
    Vh, Rh = operands(n, k)
    nan_col, inf_col = k - 1, 0
    Vh[n // 2, nan_col] = np.nan
    Vh[n - 1, inf_col] = np.inf
    V = tp.dev_matrix(Vh, dtype, dev, n + 3)
    want = singles(lo, op, V, tp.dev_matrix(Rh, dtype, dev), 2.0, -0.5)
    R = tp.dev_matrix(Rh, dtype, dev, n + 5)
    lo.mul(R, op, V, 2.0, -0.5)
    for j in range(k):
        if j in (nan_col, inf_col):
            assert not torch.isfinite(R[:, j]).any() and not torch.isfinite(want[j]).any(), j
            assert torch.equal(torch.isnan(R[:, j]), torch.isnan(want[j])), j
        else:
            assert torch.isfinite(R[:, j]).all() and same_bits(R[:, j], want[j]), j


@pytest.mark.parametrize("k", BLOCK_KS)
@pytest.mark.parametrize("n", BLOCK_NS)
def test_padding_rows_and_neighbouring_columns_keep_their_bits(lo, dev, n, k):
    """res and V are the columns 1 .. k of wider buffers with padded leading dimensions; every element outside the n x k window of
    res keeps the sentinel's bits, V is unchanged, and the window holds the vector applies"""
    dtype = torch.float64
    op = operator(lo, dev, n)
    Vh, Rh = operands(n, k)
    ldr, ldv = n + 5, n + 3
    rbuf = torch.full((ldr * (k + 2),), 7.25, dtype=dtype, device=dev)
    vbuf = torch.full((ldv * (k + 2),), NAN, dtype=dtype, device=dev)
    R = rbuf.as_strided((n, k), (1, ldr), ldr)
    V = vbuf.as_strided((n, k), (1, ldv), ldv)
    R.copy_(torch.from_numpy(Rh).to(dev))
    V.copy_(torch.from_numpy(Vh).to(dev))
    want = singles(lo, op, V, R, 2.0, -0.5)
    v0 = vbuf.clone()
    lo.mul(R, op, V, 2.0, -0.5)
    assert same_bits(vbuf, v0)
    inside = torch.zeros(ldr * (k + 2), dtype=torch.bool, device=dev)
    inside.as_strided((n, k), (1, ldr), ldr).fill_(True)
    assert (rbuf[~inside] == 7.25).all()
    for j in range(k):
        assert same_bits(R[:, j], want[j]), j


@pytest.mark.parametrize("k", BLOCK_KS)
@pytest.mark.parametrize("n", BLOCK_NS)
def test_a_block_apply_is_ldlp_block_launches_launches_and_nothing_else(lo, dev, n, k):
    dtype = torch.float64
    op = operator(lo, dev, n)
    Vh, Rh = operands(n, k)
    V, R0 = tp.dev_matrix(Vh, dtype, dev), tp.dev_matrix(Rh, dtype, dev)
    runs = []
    for _ in range(2):                                      # the first is the warm-up
        R = R0.clone(memory_format=torch.preserve_format)
        lo.mul(R, op, V, 2.0, -0.5)
        runs.append(R)
    assert same_bits(runs[0], runs[1])
    R = R0.clone(memory_format=torch.preserve_format)
    assert R.stride() == (1, n)
    gc.collect()
    torch.cuda.synchronize()
    a = tp.snap(lo)
    lo.mul(R, op, V, 2.0, -0.5)
    b = tp.snap(lo)
    torch.cuda.synchronize()
    d = {key: b[key] - a[key] for key in tp.NAMES}
    assert d["launch"] == lo.linalg.ldlp_block_launches(n, k) == -(-k // 8) * (2 * -(-n // 64) + 1), d
    assert not {key: x for key, x in d.items() if key != "launch" and x}, d
    assert same_bits(R, runs[0])


@pytest.mark.parametrize("k", BLOCK_KS)
@pytest.mark.parametrize("n", BLOCK_NS)
def test_overlap_and_short_leading_dimensions_are_refused_before_any_launch(lo, dev, n, k):
    dtype = torch.float64
    op = operator(lo, dev, n)
    half = (n + 2) * (k + 2)
    buf = torch.ones(2 * half, dtype=dtype, device=dev)
    torch.cuda.synchronize()
    p = buf.data_ptr()
    before = tp.snap(lo)
    for res, ldr in ((p + 8 * n, n),                        # res is V shifted by one column
                     (p + 8, n),                            # ... by one element
                     (p, n + 2)):                           # the same pointer, another leading dimension
        with pytest.raises(lo.MxloError, match="overlaps") as z:
            abi_block(lo, dev, op, n, res, ldr, p, n, k)
        assert z.value.status == lo._lib.EINVAL
    far = p + 8 * half                                      # no overlap: only the leading dimension is wrong
    for ldr, ldv in ((n - 1, n), (n, n - 1), (0, n)):
        with pytest.raises(lo.MxloError) as z:
            abi_block(lo, dev, op, n, far, ldr, p, ldv, k)
        assert z.value.status == lo._lib.ESHAPE
    with pytest.raises(lo.MxloError) as z:
        abi_block(lo, dev, op, n, p, n, p, n, -1)
    assert z.value.status == lo._lib.ESHAPE
    abi_block(lo, dev, op, n, p, n, p, n, 0)                # k == 0: MXLO_OK, nothing to do
    with pytest.raises(lo.MxloError, match="overlaps"):     # the same through mul!
        lo.mul(buf.as_strided((n, k), (1, n), n), op, buf.as_strided((n, k), (1, n)), 1.0, 0.0)
    after = tp.snap(lo)
    assert after == before, {key: after[key] - before[key] for key in tp.NAMES}
    torch.cuda.synchronize()
    assert torch.equal(buf, torch.ones_like(buf))


@pytest.mark.parametrize("n", BLOCK_NS)
def test_operands_of_the_wrong_shape_or_type_raise_before_any_launch(lo, dev, n):
    k = 3
    op = operator(lo, dev, n)
    good = lambda r, c, dtype=torch.float64: torch.ones((c, r), dtype=dtype, device=dev).t()
    torch.cuda.synchronize()
    before = tp.snap(lo)
    for w in (op, lo.transpose(op)):
        with pytest.raises(lo.LinearOperatorException, match="shape mismatch"):
            lo.mul(good(n, k), w, good(n + 1, k), 1.0, 0.0)
        with pytest.raises(lo.LinearOperatorException, match="shape mismatch"):
            lo.mul(good(n + 1, k), w, good(n, k), 1.0, 0.0)
        with pytest.raises(lo.LinearOperatorException, match="shape mismatch"):
            lo.mul(good(n, k + 1), w, good(n, k), 1.0, 0.0)
        for rt, vt in ((torch.float32, torch.float64), (torch.float64, torch.float32), (torch.float32, torch.float32)):
            R = good(n, k, rt)
            with pytest.raises(TypeError):
                lo.mul(R, w, good(n, k, vt), 1.0, 0.0)
            assert (R == 1).all()
    assert tp.snap(lo) == before
