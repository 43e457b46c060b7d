"""opQR, opQR(pivot=True) and opPinv (csrc/linalg.hip, linearoperators.jl_amd/linalg.py) on inputs that are hard, tied or not
finite. The inputs and the host models are tests/qr_hard_cases.py's; tests/test_qr_hard_host.py holds LAPACK and the models to
what is assumed here, on the same bits. Shapes: the smallest at which block columns (NB = 64), row chunks, the 256-thread
pivot search and the rank cut can go wrong.

1. Ill-conditioned, consistent systems: A = U diag(10^(-d i/(n-1))) V', condition number 1e10 (Float32: 1e4), at 65 x 64,
   65 x 65, 129 x 65, 200 x 129 and the transpose of each as a wide matrix, for all three operators (the pivoted two must report
   full rank). prod: eta = |v - A x| / (|A| |x| + |v|) with v = round(A x0); transposed: eta' = |A' y - u| / (|A| |y| + |u|) with a
   Gaussian u — residuals of CONSISTENT systems, so they are the normwise backward errors and are sharp where the metric of
   test_gpu_qr.py (which carries a factor |A'| more) is not. Bound: 10 eps(T). Derivation: Householder QR solves are backward
   stable with a constant of the order of one at these sizes — LAPACK's gels stays at or below 1 eps on the same operands
   (0.14 .. 0.45 eps, asserted and printed by the host file); the device runs the same algorithm with other summation orders and
   Float64 sums for both element types, for which a decade over the reference is allowed. A lost row chunk, a wrong T factor
   or a wrong block inverse costs orders of magnitude. No range-membership check: range(A) itself moves by cond eps under a
   backward perturbation; that check stays with the well-conditioned files.
2. Column scaling by powers of two commutes bit for bit through the unpivoted operator: D = diag(2^k_j), |k_j| <= 100 (20).
   A multiplication by 2^k only changes the exponent; column j of every intermediate of the factorisation carries the one
   factor 2^k_j through all terms of its sums (reflectors, tau and T are invariant), and every sum is taken in a fixed order, so
   nothing but under- or overflow can break it: the squared column norms stay within [2^-900, 2^900] (host file).
3. Uniform scaling by 2^+-E of the rank-deficient problems of test_gpu_qrp.py through the pivoted and pseudo-inverse operators:
   rank and permutation stay, both modes give the bits of the unscaled result times 2^-+E.
4. Exact pivoting with ties on monomial matrices against exact_geqp3: permutation, rank, W and both applies bit for bit.
5. Non-finite operands, and the entries an apply must not read: what the docstring of opQR promises for the basic solutions
   (the nf - r non-pivot entries are zero before the alpha, beta epilogue; the transposed mode reads u[perm[0:r]] only).

Observed maxima on an MI355X: DESIGN.md §4, the csrc/linalg.hip subsection."""
import numpy as np
import pytest
import torch

import qr_hard_cases as Q
import test_gpu_pinv as tpi
import test_gpu_qr as tq
import test_gpu_qrp as tp
from test_gpu_linalg_hard import SCALE_EXP, rounded, same_bits
from test_gpu_linalg_trees import col_major
from test_gpu_qrp import NP, dev_matrix, dev_vec, host

gpu = pytest.mark.gpu
DTYPES = [torch.float64, torch.float32]
DIDS = ["f64", "f32"]
KINDS = ["qr", "qrp", "pinv"]
MAXIMA = {}


def build(lo, kind, Ad):
    return {"qr": lo.opQR, "qrp": lambda M: lo.opQR(M, pivot=True), "pinv": lo.opPinv}[kind](Ad)


def run(lo, w, x, dtype, dev, res0=None, alpha=1.0, beta=0.0):
    """w applied to the host vector x, into a NaN-filled res unless res0 is given; the device result"""
    res = torch.full((lo.size(w, 1),), float("nan"), dtype=dtype, device=dev) if res0 is None else dev_vec(res0, dtype, dev)
    lo.mul(res, w, dev_vec(x, dtype, dev), alpha, beta)
    return res


def bits(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. ill-conditioned
def held10(tag, kind, dtype, observed):
    bound = 10 * float(torch.finfo(dtype).eps)
    key = (kind, dtype)
    MAXIMA[key] = max(MAXIMA.get(key, 0.0), observed / bound)
    print(f"{tag}: {observed:.3e} = {observed / bound:.3e} of the bound (max so far for {kind} {dtype}: {MAXIMA[key]:.3e})")
    assert observed <= bound, (tag, observed / bound)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("shape", Q.ILL_SHAPES, ids=[f"{m}x{n}" for m, n in Q.ILL_SHAPES])
@pytest.mark.parametrize("kind", KINDS)
def test_backward_error_of_ill_conditioned_consistent_systems(lo, dev, kind, shape, dtype):
    """eta, eta' <= 10 eps(T) (module docstring, 1) for A factored as it is and for its transpose as a wide matrix"""
    m, n = shape
    A, v, u, nA = Q.ill(m, n, NP[dtype])
    for wide in (False, True):
        op = build(lo, kind, dev_matrix(A.T if wide else A, dtype, dev))
        assert tuple(op.shape) == ((m, n) if wide else (n, m))
        if kind != "qr":
            assert op._rank == n, (kind, shape, wide, op._rank)
        opx, opy = (lo.transpose(op), op) if wide else (op, lo.transpose(op))
        x, y = host(run(lo, opx, v, dtype, dev)), host(run(lo, opy, u, dtype, dev))
        assert np.isfinite(x).all() and np.isfinite(y).all()
        tag = f"{kind} {m}x{n} {'wide' if wide else 'tall'} {dtype}"
        held10(f"eta {tag}", kind, dtype, Q.eta(A, nA, x, v))
        held10(f"eta' {tag}", kind, dtype, Q.eta(A.T, nA, y, u))


# ------------------------------------------------------------------------------------------------ 2. column scaling
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("shape", Q.SCALE_SHAPES, ids=[f"{m}x{n}" for m, n in Q.SCALE_SHAPES])
def test_column_scaling_by_powers_of_two_commutes_bit_for_bit(lo, dev, shape, dtype):
    """x(A D, v) D has the bits of x(A, v), y(A D, u) those of y(A, D^-1 u), through opQR(A D) and through the wide operator of
    (A D)'; W of A D is W of A with the columns of R scaled and the reflectors unchanged, T is unchanged. v is test_gpu_qr.py's
    Gaussian: NOT in the range."""
    m, n = shape
    npd = NP[dtype]
    A, v, u, _ = tq.problem(m, n, npd)
    D = np.ldexp(1.0, Q.col_exponents(n, npd))
    S = A * D[None, :]
    Dd = dev_vec(D, dtype, dev)
    ud = rounded(u / D, npd)
    plain = lo.opQR(dev_matrix(A, dtype, dev))
    x0, y0 = run(lo, plain, v, dtype, dev), run(lo, lo.transpose(plain), ud, dtype, dev)
    assert torch.isfinite(x0).all() and torch.isfinite(y0).all()
    Wp, Tp = plain._factor[0], plain._factor[1]
    for wide in (False, True):
        scaled = lo.opQR(dev_matrix(S.T if wide else S, dtype, dev))
        Ws, Ts = scaled._factor[0], scaled._factor[1]
        assert torch.equal(torch.tril(Ws, -1), torch.tril(Wp, -1)), wide                 # the reflectors
        assert torch.equal(torch.triu(Ws[:n, :]), torch.triu(Wp[:n, :]) * Dd[None, :]), wide
        assert torch.equal(Ts, Tp), wide
        opx, opy = (lo.transpose(scaled), scaled) if wide else (scaled, lo.transpose(scaled))
        assert torch.equal(run(lo, opx, v, dtype, dev) * Dd, x0), wide
        assert torch.equal(run(lo, opy, u, dtype, dev), y0), wide


# ------------------------------------------------------------------------------------------------ 3. uniform scaling
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("shape", Q.UNIFORM_SHAPES, ids=[f"{m}x{n}r{r}" for m, n, r in Q.UNIFORM_SHAPES])
@pytest.mark.parametrize("kind", ["qrp", "pinv"])
def test_uniform_scaling_keeps_rank_and_permutation_and_scales_the_bits(lo, dev, kind, shape, dtype):
    mf, nf, r = shape
    npd = NP[dtype]
    F, v, _ = tp.problem_def(*shape, npd)
    u = tpi.rhs_u(*shape, npd)
    plain = (tp.factored if kind == "qrp" else tpi.factored)(lo, dev, shape, dtype)
    assert plain._rank == r
    x0, y0 = run(lo, plain, v, dtype, dev), run(lo, lo.transpose(plain), u, dtype, dev)
    assert torch.isfinite(x0).all() and torch.isfinite(y0).all()
    for s in (SCALE_EXP[npd], -SCALE_EXP[npd]):
        scaled = build(lo, kind, dev_matrix(np.ldexp(F, s), dtype, dev))
        assert scaled._rank == r and torch.equal(scaled._perm, plain._perm), s
        back = float(np.ldexp(1.0, s))
        assert torch.equal(run(lo, scaled, v, dtype, dev) * back, x0), s
        assert torch.equal(run(lo, lo.transpose(scaled), u, dtype, dev) * back, y0), s


# ------------------------------------------------------------------------------------------------ 4. exact pivoting with ties
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("case", Q.MONOMIAL_CASES, ids=[f"{m}x{n}r{r}l{l}" for m, n, r, l in Q.MONOMIAL_CASES])
def test_exact_pivoting_with_ties_on_monomial_matrices(lo, dev, case, dtype):
    """One non-zero +-2^k per column: the factorisation and, for integer v and u, both applies are exact, so permutation, rank,
    W and the basic solutions equal exact_geqp3's bit for bit — with the first column winning every tie: all remaining
    columns at levels = 0, more of them than the pivot search has threads at nf = 300, and at norm exactly zero past the rank.
    opPinv of the deficient cases: against numpy's pinv within mf eps |pinv(F)| |v| (its second stage is not exact)."""
    mf, nf, rank, _ = case
    npd = NP[dtype]
    F, W, perm, r, taus = Q.monomial_model(case, npd)
    v, u = Q.integer_rhs(case)
    x = Q.basic_solution(W, perm, r, taus, v).astype(npd)
    y = Q.basic_solution_t(W, perm, r, taus, u).astype(npd)
    assert r == rank and not np.signbit(x[perm[r:]]).any()
    for wide in (False, True):
        op = lo.opQR(dev_matrix(F.T if wide else F, dtype, dev), pivot=True)
        got = op._perm.cpu().numpy()
        assert op._rank == r, (wide, op._rank)
        assert np.array_equal(got, perm), (wide, np.flatnonzero(got != perm)[:8], got[:8], perm[:8])
        assert same_bits(bits(op._factor[0]), W), wide
        opx, opy = (lo.transpose(op), op) if wide else (op, lo.transpose(op))
        assert same_bits(bits(run(lo, opx, v, dtype, dev)), x), wide
        assert same_bits(bits(run(lo, opy, u, dtype, dev)), y), wide
    if rank < nf:
        eps = float(torch.finfo(dtype).eps)
        X = np.linalg.pinv(F)
        nX = float(np.linalg.norm(X, 2))
        op = lo.opPinv(dev_matrix(F, dtype, dev))
        assert op._rank == r and np.array_equal(op._perm.cpu().numpy(), perm)
        tp.held(f"pinv monomial {case} {dtype}", float(np.linalg.norm(host(run(lo, op, v, dtype, dev)) - X @ v)),
                mf * eps * nX * float(np.linalg.norm(v)))
        tp.held(f"pinv' monomial {case} {dtype}", float(np.linalg.norm(host(run(lo, lo.transpose(op), u, dtype, dev)) - X.T @ u)),
                mf * eps * nX * float(np.linalg.norm(u)))


# ------------------------------------------------------------------------------------------------ 5. non-finite operands
def nonfinite_setup(lo, dev, dtype):
    shape, npd = Q.NONFINITE_SHAPE, NP[dtype]
    mf, nf, r = shape
    F, v, _ = tp.problem_def(*shape, npd)
    u = tpi.rhs_u(*shape, npd)
    res_n = rounded(np.random.default_rng(9960).standard_normal(nf), npd)
    res_m = rounded(np.random.default_rng(9961).standard_normal(mf), npd)
    assert (res_n != 0).all() and (res_m != 0).all()
    return shape, F, v, u, res_n, res_m


def poisoned(x, i, bad=float("nan")):
    out = np.array(x)
    out[i] = bad
    return out


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_a_nan_in_v_leaves_the_non_pivot_entries_of_a_basic_solution_exactly_zero(lo, dev, dtype):
    """opQR(pivot=True), prod mode: Q is dense, so the NaN reaches all r pivot entries; the nf - r others are written as
    alpha 0 + beta res, never from v: +0.0 with (1, 0), exactly -0.5 res with beta = -0.5"""
    (mf, nf, r), _, v, _, res_n, _ = nonfinite_setup(lo, dev, dtype)
    op = tp.factored(lo, dev, Q.NONFINITE_SHAPE, dtype)
    perm = op._perm.cpu().numpy()
    assert op._rank == r
    vb = poisoned(v, Q.NONFINITE_V)
    out = bits(run(lo, op, vb, dtype, dev))
    assert np.isnan(out[perm[:r]]).all()
    assert same_bits(out[perm[r:]], np.zeros(nf - r, dtype=NP[dtype]))
    out = bits(run(lo, op, vb, dtype, dev, res0=res_n, alpha=2.0, beta=-0.5))
    assert np.isnan(out[perm[:r]]).all()
    assert same_bits(out[perm[r:]], (-0.5 * res_n[perm[r:]]).astype(NP[dtype]))
    clean = bits(run(lo, op, v, dtype, dev))                    # the work space keeps nothing from the bad applies
    assert np.isfinite(clean).all() and same_bits(clean[perm[r:]], np.zeros(nf - r, dtype=NP[dtype]))


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_the_transposed_pivoted_apply_reads_only_the_pivot_entries_of_u(lo, dev, dtype):
    """y = Q[:, 0:r] inv(R11') u[perm[0:r]]: a NaN or an Inf at u[perm[j]], j >= r, is never read — the result is finite and has
    the bits of the apply with 0.0 there; a NaN at a pivot position reaches every entry (Q is dense)."""
    (mf, nf, r), _, _, u, _, res_m = nonfinite_setup(lo, dev, dtype)
    op = tp.factored(lo, dev, Q.NONFINITE_SHAPE, dtype)
    perm = op._perm.cpu().numpy()
    w = lo.transpose(op)
    free, piv = int(perm[Q.NONFINITE_FREE]), int(perm[Q.NONFINITE_PIVOT])
    want = run(lo, w, poisoned(u, free, 0.0), dtype, dev)
    assert torch.isfinite(want).all()
    for bad in (float("nan"), float("inf")):
        assert torch.equal(run(lo, w, poisoned(u, free, bad), dtype, dev), want), bad
    ub = u.copy()
    ub[perm[r:]] = np.nan                                       # and all nf - r of them at once
    assert torch.equal(run(lo, w, ub, dtype, dev), want)
    want2 = run(lo, w, poisoned(u, free, 0.0), dtype, dev, res0=res_m, alpha=2.0, beta=-0.5)
    assert torch.equal(run(lo, w, poisoned(u, free), dtype, dev, res0=res_m, alpha=2.0, beta=-0.5), want2)
    assert torch.isnan(run(lo, w, poisoned(u, piv), dtype, dev)).all()


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_a_nan_in_an_operand_of_a_dense_rectangular_solve_reaches_every_entry(lo, dev, dtype):
    """opPinv (rank 65 of 129 columns) and the unpivoted opQR, vector applies, both modes: the pseudo-inverse is dense"""
    (mf, nf, r), F, v, u, _, _ = nonfinite_setup(lo, dev, dtype)
    pinv = tpi.factored(lo, dev, Q.NONFINITE_SHAPE, dtype)
    perm = pinv._perm.cpu().numpy()
    assert pinv._rank == r
    A, va, ua, _ = tq.problem(mf, nf, NP[dtype])
    qr = tq.factored(lo, dev, (mf, nf), dtype)
    for name, op, vv, uu in (("pinv", pinv, v, u), ("qr", qr, va, ua)):
        assert torch.isnan(run(lo, op, poisoned(vv, Q.NONFINITE_V), dtype, dev)).all(), name
        for k in (int(perm[Q.NONFINITE_PIVOT]), int(perm[Q.NONFINITE_FREE]), 0, nf - 1):
            assert torch.isnan(run(lo, lo.transpose(op), poisoned(uu, k), dtype, dev)).all(), (name, k)
        assert torch.isfinite(run(lo, op, vv, dtype, dev)).all() and torch.isfinite(run(lo, lo.transpose(op), uu, dtype, dev)).all()


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("kind", KINDS)
def test_a_nan_in_res_with_beta_reaches_its_own_entry_only(lo, dev, kind, dtype):
    """res = alpha op v + beta res with (2, -0.5): a NaN at res[i] makes entry i NaN and leaves the bits of every other entry,
    in both modes; for the pivoted operator i is once a pivot entry and once one of the nf - r entries the fill writes"""
    (mf, nf, r), F, v, u, res_n, res_m = nonfinite_setup(lo, dev, dtype)
    if kind == "qr":
        op = tq.factored(lo, dev, (mf, nf), dtype)
        perm = np.arange(nf)
    else:
        op = (tp.factored if kind == "qrp" else tpi.factored)(lo, dev, Q.NONFINITE_SHAPE, dtype)
        perm = op._perm.cpu().numpy()
    for w, x, r0, spots in ((op, v, res_n, (int(perm[Q.NONFINITE_PIVOT]), int(perm[Q.NONFINITE_FREE]))),
                            (lo.transpose(op), u, res_m, (Q.NONFINITE_RES, mf - 1))):
        clean = bits(run(lo, w, x, dtype, dev, res0=r0, alpha=2.0, beta=-0.5))
        assert np.isfinite(clean).all()
        for i in spots:
            out = bits(run(lo, w, x, dtype, dev, res0=poisoned(r0, i), alpha=2.0, beta=-0.5))
            keep = np.arange(len(out)) != i
            assert np.isnan(out[i]) and same_bits(out[keep], clean[keep]), (kind, i)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("kind", KINDS)
def test_a_poisoned_column_of_a_block_apply_reaches_no_other_column(lo, dev, kind, dtype):
    """9 columns (a group of 8 and a group of 1), (alpha, beta) = (2, -0.5): column 4 carries a NaN — at a pivot position of u in the
    transposed pivoted apply — and column 8 one too; the other seven keep the bits of the clean block apply. Pivoted, prod
    mode: the non-pivot entries of the poisoned columns are exactly -0.5 res. Pivoted, transposed: a column whose only
    non-finite entries sit at non-pivot positions equals the clean one."""
    (mf, nf, r), F, v, u, res_n, res_m = nonfinite_setup(lo, dev, dtype)
    npd = NP[dtype]
    if kind == "qr":
        op = tq.factored(lo, dev, (mf, nf), dtype)
        perm = np.arange(nf)
    else:
        op = (tp.factored if kind == "qrp" else tpi.factored)(lo, dev, Q.NONFINITE_SHAPE, dtype)
        perm = op._perm.cpu().numpy()
    rng = np.random.default_rng(9970)
    for trans, nin, nout in ((False, mf, nf), (True, nf, mf)):
        w = lo.transpose(op) if trans else op
        V = rounded(rng.standard_normal((nin, 9)), npd)
        R0 = rounded(rng.standard_normal((nout, 9)), npd)
        spot = int(perm[Q.NONFINITE_PIVOT]) if trans else Q.NONFINITE_V
        Vb = V.copy()
        Vb[spot, 4] = np.nan
        Vb[spot, 8] = np.nan
        if kind == "qrp" and trans:
            Vb[perm[r:], 2] = np.inf                            # never read
        outs = []
        for M in (V, Vb):
            R = col_major(R0, dtype, dev)
            lo.mul(R, w, col_major(M, dtype, dev), 2.0, -0.5)
            outs.append(bits(R))
        clean, bad = outs
        assert np.isfinite(clean).all()
        for j in range(9):
            if j in (4, 8):
                if kind == "qrp" and not trans:
                    assert np.isnan(bad[perm[:r], j]).all()
                    assert same_bits(bad[perm[r:], j], (-0.5 * R0[perm[r:], j]).astype(npd)), (trans, j)
                else:
                    assert np.isnan(bad[:, j]).all(), (kind, trans, j)
            else:
                assert same_bits(np.ascontiguousarray(bad[:, j]), np.ascontiguousarray(clean[:, j])), (kind, trans, j)
