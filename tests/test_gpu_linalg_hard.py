"""opCholesky, opLDL, opLU and triangular opInverse (csrc/linalg.hip) on inputs that are hard, tied or not finite.

1. Ill-conditioned and graded matrices. Every diagonal block of a sweep is solved by a product with its stored explicit
   inverse, which is only conditionally backward stable; the condition is on the diagonal block.
   Triangular families (lower and upper, prod! and tprod!), sizes NB, NB + 1, 2 NB + 1, 3 NB + 1:
     randn   the triangle of a standard normal matrix (condition number 1e14 and more at these sizes),
     kahan   the Kahan matrix with theta = 1.2,
     graded  the random triangle with its columns scaled by logspace(0, -12) (Float32: logspace(0, -5)).
   Criterion: the componentwise backward error omega = max_i |T x - b|_i / (|T| |x| + |b|)_i <= n eps(T), the bound that
   substitution guarantees (Higham, Accuracy and Stability of Numerical Algorithms, Thm 8.5: gamma_n to first order). It
   is derived, not measured. The residual is evaluated in extended precision on the host, so its own rounding is not part
   of the figure. Random right-hand sides overflow Float32 on the randn and graded families, so b = round_T(T x0) with
   x0 standard normal and the product taken in Float64. The condition number of a random triangle grows like 2^n, so at
   n = 3 NB + 1 the forward error 2^n eps of a Float32 substitution passes the largest Float32: LAPACK's own Float32
   solution of randn and graded overflows there (the host file asserts that it does), and these two cases are Float64 only.
   Factorisations: A = Q diag(logspace(0, -k)) Q' symmetrised, k = 10 (Float64) / 4 (Float32), for opCholesky, for opLDL
   (A and -A: definite, so the unpivoted L D L' is as stable as Cholesky) and G = Q diag(s) V' with the same singular
   values for opLU (prod! and tprod!). Criterion: eta_inf = |A x - b|_inf / (|A|_inf |x|_inf) <= n eps(T), as in
   test_gpu_lu.py.
   Every cap is checked against LAPACK in the same precision by tests/test_linalg_hard_host.py, which imports the
   builders below, so both files see the same bits.
2. Scaling by powers of two, bit for bit.
3. Exact cases for opLU: pivot searches decided by ties, the growth matrix.
4. Right-hand sides that are not finite ("Non-finite operands").

Observed maxima on an MI355X: DESIGN.md §4, the csrc/linalg.hip subsection."""
import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
NB = 64
HARD_NS = [NB, NB + 1, 2 * NB + 1, 3 * NB + 1]
DTYPES = [torch.float64, torch.float32]
DT_IDS = ["f64", "f32"]
NP = {torch.float64: np.float64, torch.float32: np.float32}
TRI_FAMILIES = ["randn", "kahan", "graded"]
F32_OVERFLOWS = [(f, 3 * NB + 1) for f in ("randn", "graded")]     # module docstring, 1
TRI_CASES = [(f, n, t) for f in TRI_FAMILIES for n in HARD_NS for t in (np.float64, np.float32)
             if not (t is np.float32 and (f, n) in F32_OVERFLOWS)]
GRADE = {np.float64: 12, np.float32: 5}         # the columns of `graded` fall by this many decades
ILL_DECADES = {np.float64: 10, np.float32: 4}   # condition number of the ill-conditioned A and G
SCALE_EXP = {np.float64: 100, np.float32: 20}   # exponents of the power-of-two scaling are drawn from [-e, e]
TIE_N = 1100                                    # more rows than getrf_panel_kernel has threads (1024)
TIE_LATE_ROW = 1090                             # = 66 + 1024: owned by thread 66 in its SECOND stride step


def rounded(a, npd):
    return np.asarray(a, np.float64).astype(npd).astype(np.float64)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------------------------------------ builders (host only)
@functools.lru_cache(maxsize=None)
def tri_matrix(family, n, npd, upper):
    """The triangular matrix of a family in the precision the device gets, as a read-only Float64 array."""
    rng = np.random.default_rng(8100 + n)
    if family == "kahan":
        th = 1.2
        s, c = np.sin(th), np.cos(th)
        R = (np.eye(n) - c * np.triu(np.ones((n, n)), 1)) * (s ** np.arange(n))[:, None]      # upper triangular
        T = R if upper else R.T
    else:
        G = rng.standard_normal((n, n))
        T = np.triu(G) if upper else np.tril(G)
        if family == "graded":
            T = T * np.logspace(0, -GRADE[npd], n)[None, :]
    return frozen(rounded(T, npd))[0]


@functools.lru_cache(maxsize=None)
def tri_problem(family, n, npd, upper, trans):
    """(S, b): the system S x = b the apply solves, S = T or T', with b = round_T(S x0); read-only Float64 arrays."""
    T = tri_matrix(family, n, npd, upper)
    S = T.T if trans else T
    x0 = np.random.default_rng(8200 + n).standard_normal(n)
    return frozen(S, rounded(S @ x0, npd))


def omega(S, x, b):
    """componentwise backward error of x for S x = b (Oettli-Prager), the residual in extended precision"""
    Sl, xl, bl = S.astype(np.longdouble), x.astype(np.longdouble), b.astype(np.longdouble)
    r = np.abs(Sl @ xl - bl)
    den = np.abs(Sl) @ np.abs(xl) + np.abs(bl)
    ok = den > 0
    assert (r[~ok] == 0).all()
    return float((r[ok] / den[ok]).max()) if ok.any() else 0.0


@functools.lru_cache(maxsize=None)
def ill_problem(kind, n, npd):
    """(A, b) with b = round_T(A x0). kind: 'spd' (A = Q diag(s) Q', symmetrised), 'neg' (its negative), 'gen' (Q diag(s) V'),
    'gent' (the transpose of 'gen', the system tprod! solves); s = logspace(0, -k). Read-only Float64 arrays holding values of
    the device precision."""
    rng = np.random.default_rng(8300 + n)
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    V = np.linalg.qr(rng.standard_normal((n, n)))[0]
    s = np.logspace(0, -ILL_DECADES[npd], n)
    x0 = rng.standard_normal(n)
    if kind in ("gen", "gent"):
        A = (Q * s) @ V.T
    else:
        A = (Q * s) @ Q.T
        A = (A + A.T) / 2
        if kind == "neg":
            A = -A
    A = rounded(A, npd)
    if kind == "gent":
        A = np.ascontiguousarray(A.T)
    return frozen(A, rounded(A @ x0, npd))


def norm_inf(A):
    return float(np.abs(A).sum(axis=1).max())


def eta_inf(A, x, b):
    nx = np.abs(x).max()
    return float(np.abs(A @ x - b).max() / (norm_inf(A) * nx)) if nx else float(np.abs(b).max())


def growth_matrix(n):
    """W: 1 on the diagonal, -1 below it, 1 in the last column. Every pivot search is a tie between the diagonal and the
    -1s below; with the first row taken each time nothing moves and the last column doubles from row to row."""
    W = np.eye(n) - np.tril(np.ones((n, n)), -1)
    W[:, n - 1] = 1.0
    return W


def growth_factor(n):
    """the stored factor of growth_matrix(n), L strictly below the diagonal and U on and above it, in closed form"""
    F = np.eye(n) - np.tril(np.ones((n, n)), -1)
    F[:, n - 1] = 2.0 ** np.arange(n)
    return F


GROWTH_CASES = [(np.float64, NB + 1), (np.float32, NB + 1), (np.float64, 2 * NB + 1)]     # 2^128 is no Float32


def tie_matrix(n, late=None):
    """2 I with column 0 set to 1: all n candidates of the first pivot tie. late: that row of column 0 holds 3 instead."""
    A = 2.0 * np.eye(n)
    A[:, 0] = 1.0
    if late is not None:
        A[late, 0] = 3.0
    return A


def tie_factor(n):
    """the stored factor of tie_matrix(n): L[:, 0] = 1 below the diagonal, U = diag(1, 2, ..., 2)"""
    F = 2.0 * np.eye(n)
    F[:, 0] = 1.0
    return F


def same_bits(a, b):
    """two host arrays of one dtype hold the same bits (tells -0.0 from 0.0, which == does not)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    bits = {8: np.int64, 4: np.int32}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(bits), b.view(bits))


def lapack_triangular(S, b, npd, lower):
    """LAPACK's substitution in the precision npd; the result as Float64"""
    import scipy.linalg as sl
    return sl.solve_triangular(S.astype(npd), b.astype(npd), lower=lower, check_finite=False).astype(np.float64)


# ------------------------------------------------------------------------------------------------ device helpers
def dev_matrix(A, dtype, dev):
    """A on the device, column-major"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(A).T)).to(dtype).to(dev).t()


def dev_vec(x, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(dev)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def solve(lo, w, b, dtype, dev):
    """w applied to b into a NaN-filled res (beta == 0: res is not read); the result as Float64 on the host"""
    res = torch.full((len(b),), float("nan"), dtype=dtype, device=dev)
    lo.mul(res, w, dev_vec(b, dtype, dev))
    return host(res)


MAXIMA = {}


def record(key, value):
    MAXIMA[key] = max(MAXIMA.get(key, 0.0), value)
    return MAXIMA[key]


# ------------------------------------------------------------------------------------------------ 1a. triangular families
@gpu
@pytest.mark.parametrize("family,n,npd", TRI_CASES, ids=[f"{f}-{n}-{np.dtype(t).name}" for f, n, t in TRI_CASES])
def test_componentwise_backward_error_of_hard_triangular_solves(lo, dev, family, n, npd):
    """omega <= n eps(T) for the lower and the upper triangle, prod! and tprod! (module docstring, 1). Derived from
    substitution's bound, not from a run. Printed: omega / (n eps) and omega / omega_LAPACK."""
    dtype = torch.float64 if npd is np.float64 else torch.float32
    eps = float(torch.finfo(dtype).eps)
    for upper in (False, True):
        op = lo.opInverse(dev_matrix(tri_matrix(family, n, npd, upper), dtype, dev))
        assert op._triangle == ("upper" if upper else "lower")
        for trans in (False, True):
            S, b = tri_problem(family, n, npd, upper, trans)
            x = solve(lo, lo.transpose(op) if trans else op, b, dtype, dev)
            assert np.isfinite(x).all(), (family, n, upper, trans)
            w = omega(S, x, b)
            wl = omega(S, lapack_triangular(S, b, npd, lower=(upper == trans)), b)
            top = record(("omega", family, dtype), w / (n * eps))
            print(f"omega {family} {'upper' if upper else 'lower'} {'tprod' if trans else 'prod'} n={n} {dtype}: {w:.3e} = "
                  f"{w / (n * eps):.3e} n eps = {w / wl if wl else float('inf'):.3g} omega_LAPACK (max so far {top:.3e} n eps)")
            assert w <= n * eps, (family, n, dtype, upper, trans, w / (n * eps))


# ------------------------------------------------------------------------------------------------ 1b. ill-conditioned factorisations
def check_eta(tag, A, x, b, n, dtype):
    eps = float(torch.finfo(dtype).eps)
    assert np.isfinite(x).all(), tag
    e = eta_inf(A, x, b)
    top = record(("eta", tag.split()[0], dtype), e / (n * eps))
    print(f"eta_inf {tag} n={n} {dtype}: {e:.3e} = {e / (n * eps):.3e} n eps (max so far {top:.3e} n eps)")
    assert e <= n * eps, (tag, n, dtype, e / (n * eps))


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", HARD_NS)
def test_backward_error_of_ill_conditioned_cholesky_ldl_and_lu(lo, dev, n, dtype):
    """eta_inf <= n eps(T) at condition number 1e10 (Float32: 1e4), the bound of test_gpu_lu.py (derived there). opLDL
    takes A and -A, both definite; the signs of its pivots are the inertia: all +, all -."""
    npd = NP[dtype]
    A, b = ill_problem("spd", n, npd)
    check_eta("chol", A, solve(lo, lo.opCholesky(dev_matrix(A, dtype, dev)), b, dtype, dev), b, n, dtype)
    for kind, sign in (("spd", 1.0), ("neg", -1.0)):
        A, b = ill_problem(kind, n, npd)
        op = lo.opLDL(dev_matrix(A, dtype, dev))
        d = host(op._d)
        assert d.shape == (n,) and (np.sign(d) == sign).all(), (kind, int((np.sign(d) != sign).sum()))
        check_eta(f"ldl {kind}", A, solve(lo, op, b, dtype, dev), b, n, dtype)
    G, b = ill_problem("gen", n, npd)
    op = lo.opLU(dev_matrix(G, dtype, dev))
    check_eta("lu prod", G, solve(lo, op, b, dtype, dev), b, n, dtype)
    Gt, bt = ill_problem("gent", n, npd)
    assert np.array_equal(Gt.T, G)
    check_eta("lu tprod", Gt, solve(lo, lo.transpose(op), bt, dtype, dev), bt, n, dtype)


# ------------------------------------------------------------------------------------------------ 2. powers of two
def benign(n, npd):
    """(SPD M, quasi-definite K, lower Cholesky factor L of M): the well-conditioned families of test_gpu_linalg.py and
    test_gpu_ldl.py (entries between 1e-10 and 10 in magnitude, checked by the host file)"""
    rng = np.random.default_rng(8500 + n)
    G = rng.standard_normal((n, n)) / np.sqrt(n)
    M = G @ G.T + np.eye(n)
    M = rounded((M + M.T) / 2, npd)
    s = np.where(np.arange(n) % 3 == 2, -1.0, 1.0)
    K = np.where((s[:, None] < 0) & (s[None, :] < 0), -M, M)
    L = rounded(np.linalg.cholesky(M), npd)
    return M, K, L


def scaling(n, npd):
    """(exponents e, the powers 2^e) with integer e from [-SCALE_EXP, SCALE_EXP]"""
    e = np.random.default_rng(8600 + n).integers(-SCALE_EXP[npd], SCALE_EXP[npd] + 1, n)
    return e, np.ldexp(1.0, e)


@gpu
@pytest.mark.parametrize("kind", ["chol", "ldl", "lower", "upper"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_scaling_by_powers_of_two_commutes_bit_for_bit(lo, dev, dtype, kind):
    """D = diag(2^e_i). Symmetric operators: op(D A D) applied to D v equals D^-1 (op(A) applied to v); triangular ones:
    op(T D) applied to v equals D^-1 (op(T) applied to v), and transpose(op(T D)) applied to D v equals transpose(op(T))
    applied to v — with torch.equal.

    Why this is exact: a multiplication by 2^e only changes the exponent, and every operation of the factorisation and of
    the sweeps — product, fma, quotient, the square root of 4^e a, MFMA, the rounding to the storage type — gives the
    equally scaled result from equally scaled operands as long as nothing under- or overflows: each entry (i, j) of every
    intermediate carries one fixed factor 2^(+-e_i +- e_j) through all terms of its sums. Nothing under- or overflows: the
    entries of A are between 1e-10 and 10 in magnitude, so with |e_i| <= 100 (Float64) every intermediate lies within
    2^+-200 of a quantity that is at least 1e-10 eps times an entry, far from 2^-1022; with |e_i| <= 20 (Float32) within
    2^+-40, i.e. above 1e-10 * 6e-8 * 1e-12 = 6e-30 against the smallest normal Float32 1.2e-38, and the f64 work vector and
    block inverses are further away still."""
    n, npd = 2 * NB + 1, NP[dtype]
    M, K, L = benign(n, npd)
    e, D = scaling(n, npd)
    v = rounded(np.random.default_rng(8700).standard_normal(n), npd)
    Dd = dev_vec(D, dtype, dev)
    vd = dev_vec(v, dtype, dev)

    def apply(w, x):
        res = torch.full((n,), float("nan"), dtype=dtype, device=dev)
        lo.mul(res, w, x)
        return res

    if kind in ("chol", "ldl"):
        A = M if kind == "chol" else K
        ctor = lo.opCholesky if kind == "chol" else lo.opLDL
        plain, scaled = ctor(dev_matrix(A, dtype, dev)), ctor(dev_matrix(A * D[:, None] * D[None, :], dtype, dev))
        want = apply(plain, vd) / Dd
        assert torch.isfinite(want).all()
        assert torch.equal(apply(scaled, vd * Dd), want)
        if kind == "ldl":                                   # the pivots scale by 4^e
            assert torch.equal(scaled._d, plain._d * dev_vec(D * D, torch.float64, dev))
        return
    T = L if kind == "lower" else np.ascontiguousarray(L.T)
    plain, scaled = lo.opInverse(dev_matrix(T, dtype, dev)), lo.opInverse(dev_matrix(T * D[None, :], dtype, dev))
    want = apply(plain, vd) / Dd
    assert torch.isfinite(want).all()
    assert torch.equal(apply(scaled, vd), want)
    assert torch.equal(apply(lo.transpose(scaled), vd * Dd), apply(lo.transpose(plain), vd))


# ------------------------------------------------------------------------------------------------ 3. ties and growth
@gpu
@pytest.mark.parametrize("npd,n", GROWTH_CASES, ids=[f"{np.dtype(t).name}-{n}" for t, n in GROWTH_CASES])
def test_growth_matrix_every_pivot_is_a_tie_won_by_the_first_row(lo, dev, npd, n):
    """Exact in both precisions: multipliers -1, the last column doubles, U[n-1, n-1] = 2^(n-1). The first row of a tie must
    win every search, so nothing moves; the stored factor equals the closed form bit for bit. Nothing is asserted about the
    solve: the growth factor is 2^(n-1) by construction."""
    dtype = torch.float64 if npd is np.float64 else torch.float32
    op = lo.opLU(dev_matrix(growth_matrix(n), dtype, dev))
    assert np.array_equal(op._perm.cpu().numpy(), np.arange(n))
    assert same_bits(op._factor[0].cpu().numpy(), growth_factor(n).astype(npd))


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_a_tie_over_more_rows_than_the_panel_has_threads(lo, dev, dtype):
    """n = 1100, 2 I with column 0 = 1: all 1100 candidates of the first pivot tie, and row 0 must win through the stride
    of 1024, the wave butterfly and the scan over the 16 waves. Then no row moves, and every product is with 0, 1 or 2:
    the factor equals the closed form bit for bit. The solve of b = A x0 is held to eta_inf <= n eps (test_gpu_lu.py)."""
    n, npd = TIE_N, NP[dtype]
    A = tie_matrix(n)
    op = lo.opLU(dev_matrix(A, dtype, dev))
    assert np.array_equal(op._perm.cpu().numpy(), np.arange(n))
    assert same_bits(op._factor[0].cpu().numpy(), tie_factor(n).astype(npd))
    b = rounded(A @ np.random.default_rng(8800).standard_normal(n), npd)
    check_eta("tie", A, solve(lo, op, b, dtype, dev), b, n, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_the_maximum_owned_by_a_threads_second_stride_step(lo, dev, dtype):
    """the same matrix with A[1090, 0] = 3: thread 66 meets it in its second step (66 + 1024) after keeping the tied 1 of
    row 66. Past the first column the arithmetic is no longer exact: only perm[0] and the solve are asserted."""
    n, npd = TIE_N, NP[dtype]
    A = tie_matrix(n, late=TIE_LATE_ROW)
    op = lo.opLU(dev_matrix(A, dtype, dev))
    assert int(op._perm[0].item()) == TIE_LATE_ROW
    b = rounded(A @ np.random.default_rng(8801).standard_normal(n), npd)
    check_eta("late-maximum", A, solve(lo, op, b, dtype, dev), b, n, dtype)


# ------------------------------------------------------------------------------------------------ 4. non-finite right-hand sides
NONFINITE_N = 3 * NB + 1
NONFINITE_K = NB + 5


@gpu
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("triangle,trans", [("lower", False), ("upper", True), ("lower", True), ("upper", False)],
                         ids=["lower-prod", "upper-tprod", "lower-tprod", "upper-prod"])
def test_a_non_finite_entry_of_v_in_a_triangular_solve(lo, dev, triangle, trans, bad):
    """What the blocked sweep guarantees for a NaN or +Inf at v[k], M a dense well-conditioned triangle (DESIGN.md §2,
    "Non-finite operands", the paragraph on the solves): the blocks solved before the block that holds k keep the bits of
    the clean solve; entry k is not finite; for NaN every entry solved after k is NaN (as with substitution, M being dense).
    Entries of k's own block that substitution solves before k are NOT asserted: the product with the stored inverse
    multiplies its structural zeros with v[k], so they come out NaN here where substitution leaves them finite. The two
    ascending sweeps get k = NB + 5, the two descending ones the mirrored n - 1 - k. No call may raise."""
    n, dtype = NONFINITE_N, torch.float64
    L = benign(n, np.float64)[2]
    T = L if triangle == "lower" else np.ascontiguousarray(L.T)
    op = lo.opInverse(dev_matrix(T, dtype, dev))
    w = lo.transpose(op) if trans else op
    ascending = (triangle == "lower") != trans
    k = NONFINITE_K if ascending else n - 1 - NONFINITE_K
    v = rounded(np.random.default_rng(8900).standard_normal(n), np.float64)
    clean = solve(lo, w, v, dtype, dev)
    assert np.isfinite(clean).all()
    vb = v.copy()
    vb[k] = bad
    x = solve(lo, w, vb, dtype, dev)                          # a status other than OK raises MxloError in lo.mul
    torch.cuda.synchronize()
    blk = k // NB
    before = np.arange(n) < blk * NB if ascending else np.arange(n) >= (blk + 1) * NB
    after = np.arange(n) > k if ascending else np.arange(n) < k
    assert before.sum() >= NB and after.sum() >= NB
    assert same_bits(x[before], clean[before])
    assert not np.isfinite(x[k])
    if bad != bad:
        assert np.isnan(x[after]).all()
    assert same_bits(solve(lo, w, v, dtype, dev), clean)     # the work vector keeps nothing from the bad apply


@gpu
@pytest.mark.parametrize("kind", ["chol", "ldl", "lu"])
def test_a_nan_in_v_makes_every_entry_of_a_dense_solve_nan(lo, dev, kind):
    """every entry of the inverse of these dense matrices is non-zero, so one NaN in v reaches every entry of res"""
    n, dtype = 2 * NB + 1, torch.float64
    M, K, _ = benign(n, np.float64)
    A = {"chol": M, "ldl": K, "lu": np.roll(M, NB + 1, axis=0)}[kind]
    assert (np.linalg.inv(A) != 0).all()
    op = {"chol": lo.opCholesky, "ldl": lo.opLDL, "lu": lo.opLU}[kind](dev_matrix(A, dtype, dev))
    v = rounded(np.random.default_rng(8901).standard_normal(n), np.float64)
    v[NB + 5] = np.nan
    for w in (op, lo.transpose(op)):
        assert np.isnan(solve(lo, w, v, dtype, dev)).all()
