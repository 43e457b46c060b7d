"""Generators and parameter lists shared by test_gpu_complex_nonfinite.py (device) and test_complex_nonfinite_host.py (CPU):
NaN, ±Inf, signed zeros, subnormals and very large / very small magnitudes for the ComplexF64 / ComplexF32 kernels. Seeded
NumPy only; nothing here touches a GPU.

The input rules are those of test_gpu_nonfinite.py (its module docstring), applied per real component, and every builder
asserts them through `reduction_operand`:
  * a reduction sees Infs of ONE sign only, or an explicit +Inf / -Inf pair;
  * scaled data stays <= 1e120 (1e15 for ComplexF32) and >= 1e-120 (1e-15); scaled vectors are at most 2^16 long;
  * no component that multiplies an Inf is exactly zero — except in the named `zero_component` / `inf_zero` / `inf_azero`
    cases, whose whole point is the one-sided NaN of `(a + 0i) * (Inf + yi)` (base/complex.jl multiplies component by
    component, no recovery; oracle/lo_oracle_cplx.h restates that).
Each builder of a reducing family returns `(operands, expectations)`: the operands as NumPy arrays and a dict of facts
that must hold on the ORACLE's result (`assert_expectations`), so that a case cannot decay into one that no longer
discriminates."""
import numpy as np

from test_gpu_nonfinite import DOWN, UP, reduction_operand, special_values, unit_mags

CDTS = (np.complex128, np.complex64)
RD = {np.complex128: np.float64, np.complex64: np.float32}


def rview(a):
    a = np.ascontiguousarray(a)
    return a.view(a.real.dtype) if a.dtype.kind == "c" else a


# =========================================================================== elementwise leaves
LEAF_SIZES = (1, 3, 64, 257, 4099)
LEAF_FAMILIES = ("diag", "diag_H", "diag_rect", "diag_rect_H", "eye", "eye_rect", "zeros", "scale", "conj", "restrict_extend")


def cpattern(npd, n, which, shift):
    """Complex vector whose real and imaginary components walk `special_values` at different rates: the real part as
    test_gpu_nonfinite.pattern does, the imaginary part 7 steps further per period (7 is coprime to the 18 values), so
    every (re, im) pair of values meets within 18^2 = 324 elements; `which` = 0, 1, 2 (the three operands of a leaf) walk at
    different rates too, the imaginary part moves one more step per 324 elements (so a component of one operand meets
    every value of either component of another within n = 4099) and `shift` moves the start."""
    sv = special_values(RD[npd])
    L = sv.size
    i = np.arange(n) + shift
    out = np.empty(n, npd)
    out.real = sv[(i + which * (i // L) + 5 * which) % L]
    out.imag = sv[(i + (7 + which) * (i // L) + i // (L * L) + 5 * which + 1) % L]
    return out


REAL_ALPHAS = (1.0, 0.0, -0.0, -1.0, 2.0, 3.0)
COMPLEX_ALPHAS = (complex(1, 0), complex(0, 0), complex(0, -0.0), complex(-0.0, 0), complex(0, 1), 2 + 3j, 0.5 - 1j)
# the three classes of β each α meets once
ZERO_BETAS = (0.0, -0.0, complex(0, 0), complex(0, -0.0), complex(-0.0, 0))
REAL_BETAS = (1.0, -1.0, 2.0, 3.0)
COMPLEX_BETAS = (complex(1, 0), complex(0, 1), 2 + 3j, 0.5 - 1j)


def _as32(x):
    return np.complex64(x) if isinstance(x, complex) else np.float32(x)


def scalar_variants(npd):
    """(α, β): every real and every complex α with a zero β, a real non-zero β and a complex non-zero β (the β of each class
    rotates through its list). ComplexF64: Python scalars (Float64 / ComplexF64). ComplexF32: those (Julia's mixed
    precision) and then the np.float32 / np.complex64 versions of the same."""
    out = []
    for k, a in enumerate(REAL_ALPHAS + COMPLEX_ALPHAS):
        for betas in (ZERO_BETAS, REAL_BETAS, COMPLEX_BETAS):
            out.append((a, betas[k % len(betas)]))
    if npd == np.complex64:
        out += [(_as32(a), _as32(b)) for a, b in out]
    return out


def is_zero(b):
    return complex(b) == 0


def scalar_spellings_differ(npd):
    """(α, β): does the ORACLE's opDiagonal result on the pattern differ between the Real spelling 1.0 and Complex(1, 0) of α
    (of β) for at least one leaf size? A Real scalar multiplies component by component; (1 + 0i) * (Inf + yi) has
    0 * Inf = NaN in its imaginary part. If the two never differ, the pattern is too weak to see a kernel that ignores
    the real-scalar flag or applies it to the wrong scalar."""
    import oracle
    seen = [False, False]
    for n in LEAF_SIZES:
        d, v, r0 = (cpattern(npd, n, w, 0) for w in range(3))
        for k, (real, cplx) in enumerate((((1.0, 2.0), (complex(1, 0), 2.0)), ((2.0, 1.0), (2.0, complex(1, 0))))):
            wr = oracle.diag_mul(r0.copy(), d, v, *real, flags=oracle.scalar_flags(npd, *real))
            wc = oracle.diag_mul(r0.copy(), d, v, *cplx, flags=oracle.scalar_flags(npd, *cplx))
            seen[k] = seen[k] or not np.array_equal(class_map(wr), class_map(wc))
    return tuple(seen)


def cunit_mags(rng, shape, npd):
    """both components: random sign, magnitude in [0.5, 1] — no zero component, room for both scale factors."""
    rd = RD[npd]
    out = np.empty(shape, npd)
    out.real = unit_mags(rng, shape, rd)
    out.imag = unit_mags(rng, shape, rd)
    return out


def _set(x, idx, re=None, im=None):
    z = x[idx]
    x[idx] = complex(z.real if re is None else re, z.imag if im is None else im)


def _no_zero_component(*arrs):
    for a in arrs:
        assert not (rview(a) == 0).any(), "a zero component would multiply an Inf"


def assert_expectations(want, exp, what=""):
    """The facts of `exp` on an oracle result (a complex vector)."""
    w = rview(want)
    if exp.get("all_nan"):
        assert np.isnan(w).all(), what
    if exp.get("all_finite"):
        assert np.isfinite(w).all(), what
    if exp.get("no_nan"):
        assert not np.isnan(w).any(), what
    if "finite_at" in exp:                                # real-view indices: exactly these components are finite
        assert np.array_equal(np.flatnonzero(np.isfinite(w)), np.sort(np.asarray(exp["finite_at"], np.int64))), what
    if "inf_except" in exp:                               # every component is ±Inf except these real-view indices (finite)
        keep = np.ones(w.size, bool)
        keep[list(exp["inf_except"])] = False
        assert np.isinf(w[keep]).all() and np.isfinite(w[~keep]).all(), what
    if "n_nonfinite" in exp:
        assert int((~np.isfinite(w)).sum()) == exp["n_nonfinite"], what
    if "nan_at" in exp:                                   # real-view indices: exactly these components are NaN
        assert np.array_equal(np.flatnonzero(np.isnan(w)), np.sort(np.asarray(exp["nan_at"], np.int64))), what
    if exp.get("some_finite"):
        assert np.isfinite(w).any(), what


# the three (α, β) pairs of the reducing families: real with β = 0, real, complex
PAIRS = ((1.0, 0.0), (3.0, -4.0), (0.5 - 1j, 2 + 0.25j))


def real_pair(a, b):
    return not isinstance(a, complex) and not isinstance(b, complex)


# =========================================================================== Householder
HOUSE_CASES = ("nan_h", "inf_re_v", "inf_im_v", "inf_pair_v", "big_v", "small_v")
HOUSE_SIZES = (64, 257, 1025, 4099)                 # 1025: the smallest n whose dot takes two workgroups (4 * 256 elements each)


def house_case(npd, n, case, p, rng):
    """h (unit norm, no zero component), v and what the rules fix: NaN in Re(h[p]) — the dot is NaN, everything is NaN;
    one Inf in Re(v[p]) / Im(v[p]) — the dot's components hold one Inf each; a +Inf / -Inf pair in Re(v) opposite
    h components of one sign — NaN in every order; v scaled up / down — finite."""
    h = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    hr = rview(h)
    hr[hr == 0] = 0.5
    h = (h / np.linalg.norm(h)).astype(npd)
    v = cunit_mags(rng, n, npd)
    exp = {}
    if case == "nan_h":
        _set(h, p, re=np.nan)
        exp = {"all_nan": True}
    elif case == "inf_re_v":
        _set(v, p, re=np.inf)
    elif case == "inf_im_v":
        _set(v, p, im=np.inf)
    elif case == "inf_pair_v":
        q = (p + n // 3) % n
        q = q if q != p else (p + 1) % n
        assert q != p, "the pair needs two positions"
        h[p], h[q] = complex(abs(h[p].real), abs(h[p].imag)), complex(abs(h[q].real), abs(h[q].imag))
        _set(v, p, re=np.inf)
        _set(v, q, re=-np.inf)
        exp = {"all_nan": True}
    elif case == "big_v":
        v = (v * UP(RD[npd])).astype(npd)
        exp = {"all_finite": True}
    elif case == "small_v":
        v = (v * DOWN(RD[npd])).astype(npd)
        exp = {"all_finite": True}
    else:
        raise KeyError(case)
    _no_zero_component(h[np.isfinite(h)], v[np.isfinite(v)])
    reduction_operand(h, npd), reduction_operand(v, npd, scaled=case in ("big_v", "small_v"))
    return (h, v), exp


# =========================================================================== dense GEMV
GEMV_SHAPES = ((10, 6), (300, 257), (64, 2000), (520, 260))
GEMV_CASES = ("nan_x", "inf_re_x", "inf_im_x", "nan_M", "ninf_im_M", "zero_component", "big_x", "small_x")
GEMV_MODES = ("N", "T", "C", "J")                       # J: conj(M)*v — what the row-major alias of M' runs


def band_shape(npd, num_cu):
    """The smallest shape `cgemv_rows_band` admits (csrc/complex.hip): m >= 8 * VR * num_cu rows, n >= 1024 columns, aligned;
    VR = 16 / sizeof(element)."""
    return 8 * (16 // np.dtype(npd).itemsize) * num_cu, 1024


def gemv_case(npd, M, x, mode, case):
    """Copies of (M, x) with the case applied; x has the length the mode reads (n for N / J, m for T / C)."""
    m, n = M.shape
    rows = mode in ("N", "J")
    nin = n if rows else m
    assert x.size == nin
    M, x = M.copy(), x.copy()
    exp = {}
    p = nin - 1
    if case == "nan_x":
        _set(x, nin // 2, re=np.nan)
        exp = {"all_nan": True}
    elif case == "inf_re_x":
        _set(x, p, re=np.inf)
    elif case == "inf_im_x":
        _set(x, p, im=np.inf)
    elif case == "nan_M":
        M[m // 2, n - 1] = complex(np.nan, M[m // 2, n - 1].imag)
        exp = {"nan_rows": [m // 2 if rows else n - 1]}
    elif case == "ninf_im_M":
        M[m - 1, n // 2] = complex(M[m - 1, n // 2].real, -np.inf)
    elif case == "zero_component":                       # M entry a + 0i opposite the Inf in Re(x[p]): NaN in Im of that output only
        _set(x, p, re=np.inf)
        o = (m if rows else n) // 3
        ij = (o, p) if rows else (p, o)
        M[ij] = complex(M[ij].real, 0.0)
        exp = {"nan_at_real_pair": [2 * o + 1]}
    elif case == "big_x":
        x = (x * UP(RD[npd])).astype(npd)
        exp = {"all_finite": True}
    elif case == "small_x":
        x = (x * DOWN(RD[npd])).astype(npd)
        exp = {"all_finite": True}
    else:
        raise KeyError(case)
    if case != "zero_component":
        _no_zero_component(M[np.isfinite(M)])
    else:
        assert int((rview(M) == 0).sum()) == 1
    reduction_operand(M, npd), reduction_operand(x, npd, scaled=case in ("big_x", "small_x"))
    return (M, x), exp


def assert_gemv_expectations(want, exp, a, b, what=""):
    assert_expectations(want, exp, what)
    w = rview(want)
    if "nan_rows" in exp:
        r = exp["nan_rows"][0]
        assert np.array_equal(np.flatnonzero(np.isnan(w)), [2 * r, 2 * r + 1]), what
    if "nan_at_real_pair" in exp and real_pair(a, b):
        assert np.array_equal(np.flatnonzero(np.isnan(w)), exp["nan_at_real_pair"]), what
        assert not np.isfinite(w).any(), what


# =========================================================================== opHermitian
HERM_SIZES = {np.complex128: (5, 129, 257), np.complex64: (5, 257, 515)}   # ragged only | one DSEL block + ragged | interior strips
HERM_CASES = ("nan_v", "inf_re_v", "ninf_im_v", "nan_d", "inf_L", "big_v")
HERM_PARAMS = [(npd, n, d_real, aligned) for npd in CDTS for n in HERM_SIZES[npd] for d_real in (True, False)
               for aligned in (True, False)]


def herm_base(npd, n, d_real, seed):
    """(d, A, v, r0): A holds NaN + NaN i on and above the diagonal (it must never surface) and no zero component below;
    d real or complex without a zero component."""
    rng = np.random.default_rng(seed)
    A = cunit_mags(rng, (n, n), npd)
    A[np.triu_indices(n)] = complex(np.nan, np.nan)
    d = unit_mags(rng, n, RD[npd]) if d_real else cunit_mags(rng, n, npd)
    v = cunit_mags(rng, n, npd)
    r0 = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(npd)
    return d, A, v, r0


def herm_case(npd, base, case, a, b):
    """Copies of (d, A, v) with the case applied, and the class map the rules fix for real (α, β)."""
    d, A, v, _ = base
    n = v.size
    d, A, v = d.copy(), A.copy(), v.copy()
    d_real = d.dtype.kind != "c"
    k = n // 2
    exp = {}
    rp = real_pair(a, b)
    if case == "nan_v":
        _set(v, k, re=np.nan)
        # real d, real scalars: d_k * (NaN + y i) leaves the imaginary part of row k finite, the only finite component;
        # a complex d or a complex scalar mixes the NaN into both components there too
        exp = {"finite_at": [2 * k + 1]} if d_real and rp else {"all_nan": True}
    elif case in ("inf_re_v", "ninf_im_v"):
        if case == "inf_re_v":
            _set(v, k, re=np.inf)
        else:
            _set(v, k, im=-np.inf)
        if rp:
            exp = {"no_nan": True, "inf_except": [2 * k + (1 if case == "inf_re_v" else 0)] if d_real else []}
    elif case == "nan_d":
        if d_real:
            d[n - 1] = np.nan
        else:
            _set(d, n - 1, re=np.nan)
        exp = {"nan_at": [2 * n - 2, 2 * n - 1]}
    elif case == "inf_L":
        _set(A, (n - 2, n // 3), re=np.inf)
        if rp:
            exp = {"n_nonfinite": 4, "no_nan": True}
    elif case == "big_v":
        v = (v * UP(RD[npd])).astype(npd)
        exp = {"all_finite": True}
    else:
        raise KeyError(case)
    L = np.tril(A, -1)
    _no_zero_component(L[np.tril_indices(n, -1)][np.isfinite(L[np.tril_indices(n, -1)])], d[np.isfinite(d)])
    reduction_operand(L, npd), reduction_operand(d, npd), reduction_operand(v, npd, scaled=case == "big_v")
    return (d, A, L, v), exp


def defect_model(d, L, v, a, b, r0):
    """What a kernel computes that zeroes the elements on and above the diagonal and then multiplies them by v all the
    same: the DENSE products with tril(A, -1), its zeros included — 0 * Inf = NaN appears in rows and columns the stored
    triangle never touches. (NumPy's complex multiply is component by component, like the reference's.)"""
    with np.errstate(all="ignore"):
        n = v.size
        t1 = np.zeros(n, np.complex128)
        t2 = np.zeros(n, np.complex128)
        Lc = L.astype(np.complex128)
        vc = v.astype(np.complex128)
        for j in range(n):
            t1 += _cmul(Lc[:, j], vc[j])
        for i in range(n):
            t2 += _cmul(np.conj(Lc[i, :]), vc[i])
        dv = _cmul(d.astype(np.complex128), vc) if d.dtype.kind == "c" else _rscale(vc, d.astype(np.float64))
        inner = (dv + t1) + t2
        out = inner * a if isinstance(a, complex) else _rscale(inner, a)
        if complex(b) != 0:
            out = out + (r0 * b if isinstance(b, complex) else _rscale(r0.astype(np.complex128), b))
        return out


def _cmul(x, y):
    """component-by-component complex product (no Inf recovery)."""
    y = np.asarray(y, np.complex128)
    out = np.empty(np.broadcast(x, y).shape, np.complex128)
    out.real = x.real * y.real - x.imag * y.imag
    out.imag = x.real * y.imag + x.imag * y.real
    return out


def _rscale(z, s):
    out = np.empty(z.shape, np.complex128)
    out.real, out.imag = z.real * s, z.imag * s
    return out


def class_map(x):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf per real component."""
    w = rview(np.asarray(x))
    return np.where(np.isnan(w), 1, np.where(w == np.inf, 2, np.where(w == -np.inf, 3, 0)))


# =========================================================================== sparse
SPARSE_CASES = ("nan", "inf_re", "inf_im", "inf_zero", "inf_azero", "inf_nz")
SPARSE_MODES = ("N", "T", "C")


def sparse_matrix(npd):
    """The matrix of test_gpu_nonfinite.test_sparse_nonfinite with complex values: 3500 x 2600, column 5 stores 3000 entries
    and row 11 stores 2594 (a chunk is 2048); the first stored entry of column 3 is 0 + 0i, that of column 4 is a + 0i."""
    rng = np.random.default_rng(9)
    m, n = 3500, 2600
    cols = []
    for j in range(n):
        k = 3000 if j == 5 else 1 + (j % 6)
        cols.append(np.sort(rng.choice(m, k, replace=False)))
    cols[6] = np.union1d(cols[6], [11])
    for j in range(7, n):
        cols[j] = np.union1d(cols[j], [11])
    colptr = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int64)
    rowval = np.concatenate(cols).astype(np.int64)
    nz = cunit_mags(rng, rowval.size, npd)
    zero_col, azero_col = 3, 4
    nz[colptr[zero_col]] = 0
    nz[colptr[azero_col]] = complex(nz[colptr[azero_col]].real, 0.0)
    zero_row, azero_row = int(rowval[colptr[zero_col]]), int(rowval[colptr[azero_col]])
    assert len({zero_row, azero_row, 11}) == 3 and int((rview(nz) == 0).sum()) == 3
    colidx = np.repeat(np.arange(n), np.diff(colptr))
    return dict(m=m, n=n, colptr=colptr, rowval=rowval, nz=nz, colidx=colidx, zero=(zero_row, zero_col),
                azero=(azero_row, azero_col), long_col=5, long_row=11)


def sparse_case(npd, S, x, mode, case):
    """(nz, x) copies with the case applied. The vector position sits opposite the long column / row for "nan", opposite an
    ordinary column for the Infs and opposite the stored zero / a + 0i for the two zero cases."""
    trans = mode != "N"
    nz, x = S["nz"].copy(), x.copy()
    exp = {"some_finite": True}
    pick = lambda rc: rc[0] if trans else rc[1]
    if case == "nan":
        _set(x, S["long_row"] if trans else S["long_col"], re=np.nan)
    elif case == "inf_re":
        _set(x, S["long_row"] if trans else 9, re=np.inf)
    elif case == "inf_im":
        _set(x, S["long_row"] if trans else 9, im=np.inf)
    elif case == "inf_zero":                              # 0 + 0i opposite the Inf: NaN in both components there, nowhere else
        _set(x, pick(S["zero"]), re=np.inf)
        o = S["zero"][1] if trans else S["zero"][0]
        exp["nan_at_real_pair"] = [2 * o, 2 * o + 1]
    elif case == "inf_azero":                             # a + 0i opposite the Inf: NaN in the imaginary component there
        _set(x, pick(S["azero"]), re=np.inf)
        o = S["azero"][1] if trans else S["azero"][0]
        exp["nan_at_real_pair"] = [2 * o + 1]
    elif case == "inf_nz":
        q = S["colptr"][100] + 1                          # an ordinary stored value
        nz[q] = complex(np.inf, nz[q].imag)
    else:
        raise KeyError(case)
    reduction_operand(nz, npd), reduction_operand(x, npd)
    return (nz, x), exp


def sparse_scale(S, nz, x, mode):
    """(|A| |x|).max() over the finite part of the operands — the scale of test_gpu_sparse.py's bound."""
    xa = np.abs(np.where(np.isfinite(x), x, 0).astype(np.complex128))
    na = np.abs(np.where(np.isfinite(nz), nz, 0).astype(np.complex128))
    out = np.zeros(S["n"] if mode != "N" else S["m"])
    if mode != "N":
        np.add.at(out, S["colidx"], na * xa[S["rowval"]])
    else:
        np.add.at(out, S["rowval"], na * xa[S["colidx"]])
    return float(out.max())


# =========================================================================== real operators on complex vectors
REAL_ON_COMPLEX = ("dense", "dense_T", "hermitian", "sparse", "kron", "blockdiag")
PLANE_POISONS = (("re", np.inf), ("re", np.nan), ("im", np.inf), ("im", np.nan))
