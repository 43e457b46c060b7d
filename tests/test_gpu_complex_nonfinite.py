"""-m gpu: NaN, ±Inf, signed zeros, subnormals and very large / very small magnitudes through the ComplexF64 / ComplexF32
kernels (csrc/complex.hip, the complex instantiations of sparse.hip, the real-operator-on-complex-vector path of
operators.py), against the oracle's component-by-component restatement of Julia's complex arithmetic
(oracle/lo_oracle_cplx.h).

Rules of comparison and of the inputs: those of test_gpu_nonfinite.py (`check_against_oracle`, `reduction_operand`), per
real component. The generators and parameter lists live in complex_nonfinite_cases.py; test_complex_nonfinite_host.py
checks them (and the oracle's expectations) without a GPU.

Tolerances — no new numbers: on the oracle's finite positions each family uses the bound of the finite-data test that owns it
(named next to each constant).

Out of scope: the `MXLO_SPARSE_COMPLEX_PLANES=1` environment switch (opt-in, read at construction; its finite-data parity
is test_gpu_sparse.py::test_complex_sparse_operator_native_and_through_real_planes)."""
import numpy as np
import pytest
import torch

import oracle
import complex_nonfinite_cases as cc
from test_gpu_nonfinite import (HOUSE_FORMS, T, TM, TOL_CHOUSE, TOL_GEMV, TOL_HERM, TOL_KRON, TOL_SPARSE, check_against_oracle,
                                launches, put, unit_mags)      # (the BIG / SMALL / UP / DOWN rules: through the case builders)

pytestmark = pytest.mark.gpu

TD = {np.complex128: torch.complex128, np.complex64: torch.complex64}
TR = {np.complex128: torch.float64, np.complex64: torch.float32}
CDT_IDS = ["c128", "c64"]
# TOL_CHOUSE (1e-12 / 1e-5, defined in test_gpu_nonfinite.py): test_gpu_complex.py::test_complex_householder_parity
# TOL_GEMV, TOL_HERM, TOL_KRON, TOL_SPARSE (the real families under the planes of a complex vector): cited where they are defined
TOL_CGEMV = {np.complex128: 1e-12, np.complex64: 3e-5}   # test_gpu_complex.py::test_complex_dense_gemv_all_modes_both_layouts
TOL_CHERM = {np.complex128: 1e-12, np.complex64: 3e-5}   # test_gpu_complex.py::test_complex_hermitian_parity / _strip_regimes
# test_gpu_sparse.py::test_complex_sparse_operator_native_and_through_real_planes: max abs <= 8 * tol * (|a| (|A| |v|).max() + |b| max|res|)
TOL_CSPARSE = {np.complex128: 8 * 1e-13, np.complex64: 8 * 5e-6}
NANC = complex(float("nan"), float("nan"))


def result_buffer(r0, dev, off, b):
    """res on the device: r0, or NaN + NaN i where β is a zero (res must not be read)."""
    res = put(r0, dev, off)
    if cc.is_zero(b):
        res.fill_(NANC)
    return res


# =========================================================================== a. elementwise leaves, bit for bit
@pytest.mark.parametrize("npd", cc.CDTS, ids=CDT_IDS)
@pytest.mark.parametrize("family", cc.LEAF_FAMILIES)
def test_complex_elementwise_leaves_special_values_bit_exact(lo, dev, npd, family):
    """opDiagonal (square, adjoint, rectangular both ways and their adjoints), opEye (square, rectangular both ways),
    opZeros, `res .*= α`, conj (in and out of place), restriction and extension on complex vectors whose components walk ±0,
    ±Inf, NaN, subnormals, the smallest normal, the largest finite and ordinary values: the oracle's bits, for aligned
    operands and for views one element into a buffer (an 8-byte phase for ComplexF32), for every real and complex spelling
    of α and β — a Real scalar multiplies component by component (complex_scalars.h), which differs from Complex(x, 0) in
    signed zeros and non-finite values; `scalar_spellings_differ` shows that this data tells the two apart."""
    from linearoperators_jl_amd import operators
    dtype = TD[npd]
    S = lo.Storage(dtype, dev)
    if family == "diag":
        assert cc.scalar_spellings_differ(npd) == (True, True), "the pattern cannot tell 1.0 from complex(1, 0)"
    for n in cc.LEAF_SIZES:
        for off in (0, 1):
            for k, (a, b) in enumerate(cc.scalar_variants(npd)):
                fl = oracle.scalar_flags(npd, a, b)
                d, v, r0 = (cc.cpattern(npd, n, w, k + off) for w in range(3))
                what = str((family, n, off, a, b))
                if family in ("diag", "diag_H"):
                    cj = family == "diag_H"
                    D = lo.opDiagonal(put(d, dev, off))
                    res = result_buffer(r0, dev, off, b)
                    lo.mul(res, D.H if cj else D, put(v, dev, off), a, b)
                    want = oracle.diag_mul(r0.copy(), d, v, a, b, flags=fl | (oracle.CONJ_D if cj else 0))
                    check_against_oracle(res.cpu().numpy(), want, bitwise=True, what=what)
                elif family in ("diag_rect", "diag_rect_H"):         # tail rows are zeroed whatever β is
                    cj = family == "diag_rect_H"
                    for nrow, ncol in ((n + 2, n), (n, n + 2)):
                        Dr = lo.opDiagonal(nrow, ncol, put(d, dev, off))
                        nin, nout = (nrow, ncol) if cj else (ncol, nrow)
                        vin, rr = cc.cpattern(npd, nin, 1, k + off), cc.cpattern(npd, nout, 2, k + off)
                        res = result_buffer(rr, dev, off, b)
                        lo.mul(res, Dr.H if cj else Dr, put(vin, dev, off), a, b)
                        want = oracle.diag_mul(rr.copy(), d, vin[:n].copy(), a, b, n_min=n, flags=fl | (oracle.CONJ_D if cj else 0))
                        check_against_oracle(res.cpu().numpy(), want, bitwise=True, what=what + str((nrow, ncol)))
                elif family == "eye":
                    res = result_buffer(r0, dev, off, b)
                    lo.mul(res, lo.opEye(dtype, n, S=S), put(v, dev, off), a, b)
                    want = oracle.eye_mul(r0.copy(), v, a, b, flags=fl | oracle.TAIL_BETA)
                    check_against_oracle(res.cpu().numpy(), want, bitwise=True, what=what)
                elif family == "eye_rect":
                    for nrow, ncol in ((n + 2, n), (n, n + 2)):
                        vin, rr = cc.cpattern(npd, ncol, 1, k + off), cc.cpattern(npd, nrow, 2, k + off)
                        res = result_buffer(rr, dev, off, b)
                        lo.mul(res, lo.opEye(dtype, nrow, ncol, S=S), put(vin, dev, off), a, b)
                        want = oracle.eye_mul(rr.copy(), vin, a, b, n_min=n, flags=fl | oracle.TAIL_BETA)
                        check_against_oracle(res.cpu().numpy(), want, bitwise=True, what=what + str((nrow, ncol)))
                elif family == "zeros":
                    res = result_buffer(r0, dev, off, b)
                    lo.mul(res, lo.opZeros(dtype, n, n, S=S), put(v, dev, off), a, b)
                    want = oracle.zeros_mul(r0.copy(), b, flags=fl)
                    check_against_oracle(res.cpu().numpy(), want, bitwise=True, what=what)
                elif family == "scale":
                    res = put(r0, dev, off)
                    operators._scale(res, a)
                    want = oracle.scale(r0.copy(), a, flags=oracle.scalar_flags(npd, a, 0))
                    check_against_oracle(res.cpu().numpy(), want, bitwise=True, what=what)
                elif family == "conj":                               # flips the sign of every imaginary component, zeros included
                    if k >= 2:
                        continue
                    want = v.copy()
                    want.imag = -v.imag
                    if k == 0:
                        res = operators.conj_into(put(r0, dev, off), put(v, dev, off))
                    else:
                        res = put(v, dev, off)
                        operators.conj_into(res, res)
                    check_against_oracle(res.cpu().numpy(), want, bitwise=True, what=what)
                    assert np.array_equal(np.signbit(res.cpu().numpy().imag), ~np.signbit(v.imag)), what
                else:                                                # restriction / extension move bytes: NaN payloads included
                    if k >= 2:
                        continue
                    rng = np.random.default_rng(n + k)
                    idx = (rng.integers(1, n + 1, max(1, n // 2)) if k == 0 else np.flatnonzero(rng.random(n) < 0.6) + 1).astype(np.int64)
                    if idx.size == 0:
                        idx = np.array([1], np.int64)
                    P = lo.opRestriction(idx, n, device=dev)
                    out = put(np.full(idx.size, 7, npd), dev, off)
                    lo.mul(out, P, put(v, dev, off))
                    u8 = lambda x: np.ascontiguousarray(x).view(np.uint8)
                    assert np.array_equal(u8(out.cpu().numpy()), u8(v[idx - 1])), what
                    back = put(r0, dev, off)
                    lo.mul(back, P.H, put(v[:idx.size].copy(), dev, off))
                    wantb = oracle.extend(np.empty(n, npd), v[:idx.size].copy(), idx)
                    assert np.array_equal(u8(back.cpu().numpy()), u8(wantb)), what


# =========================================================================== b. Householder
@pytest.mark.parametrize("npd", cc.CDTS, ids=CDT_IDS)
@pytest.mark.parametrize("form", list(HOUSE_FORMS))
def test_complex_householder_nonfinite_every_form(lo, dev, npd, form):
    """mulHouseholder! on complex data under every setting of the launch-form keys of the real kernel (`HOUSE_FORMS`). The
    complex instantiation (complex.hip: chouse) reads none of them and has ONE schedule for every n > 0 — the conjugated
    dot's partials pass, its finalize launch, the update: exactly 3 launches are witnessed at every size and under every
    setting, and the keys must not change what is computed. n = 64, 257 (one workgroup in the dot), 1025 (the smallest n
    with two: a workgroup covers 4 * 256 elements) and 4099. NaN in Re(h) (all NaN), one Inf in Re(v) / Im(v), a +Inf / -Inf
    pair in Re(v) (all NaN), v scaled up and down (finite, TOL_CHOUSE); the special element in the first chunk and at the end."""
    ctx = lo.get_ctx(dev)
    fused, inline_n, _ = HOUSE_FORMS[form]
    rng = np.random.default_rng(77)
    with ctx.tuned(house_fused=fused, house_inline_n=inline_n):
        for n in cc.HOUSE_SIZES:
            for case in cc.HOUSE_CASES:
                for p in ((5,) if case in ("big_v", "small_v") else (5, n - 1)):
                    (h, v), exp = cc.house_case(npd, n, case, p, rng)
                    r0 = cc.cunit_mags(rng, n, npd)
                    H = lo.opHouseholder(T(h, dev))
                    for a, b in cc.PAIRS:
                        res = result_buffer(r0, dev, 0, b)
                        l0 = launches(lo)
                        lo.mul(res, H, T(v, dev), a, b)
                        nl = launches(lo) - l0
                        assert nl == 3, (form, n, nl)
                        want = oracle.householder_mul(r0.copy(), h, v, a, b, flags=oracle.scalar_flags(npd, a, b))
                        cc.assert_expectations(want, exp, str((n, case, p)))
                        check_against_oracle(res.cpu().numpy(), want, tol=TOL_CHOUSE[npd], what=str((form, n, case, p, a, b)))
    ctx.sync()


# =========================================================================== c. dense GEMV
def _gemv_modes(lo, dev, Mc):
    """the four device operators of one stored matrix: N, T, C on column-major storage, and conj(M)*x (J) as the adjoint of
    the row-major alias of transpose(M)."""
    op = lo.LinearOperatorFromMatrix(TM(Mc, dev))
    alias = lo.LinearOperatorFromMatrix(T(np.ascontiguousarray(Mc.T), dev))          # torch row-major n x m == column-major m x n
    return {"N": op, "T": op.T, "C": op.H, "J": alias.H}


def _run_gemv(lo, dev, npd, m, n, band=False):
    rng = np.random.default_rng(m * 7 + n)
    M = cc.cunit_mags(rng, (m, n), npd)
    xs = {True: cc.cunit_mags(rng, n, npd), False: cc.cunit_mags(rng, m, npd)}
    for case in cc.GEMV_CASES:
        ops, Mcur = None, None
        for mode in cc.GEMV_MODES:
            rows = mode in ("N", "J")
            (Mc, xc), exp = cc.gemv_case(npd, M, xs[rows], mode, case)
            if ops is None or not np.array_equal(cc.rview(Mc), cc.rview(Mcur), equal_nan=True):
                ops, Mcur = _gemv_modes(lo, dev, Mc), Mc
            nout = m if rows else n
            r0 = cc.cunit_mags(rng, nout, npd)
            for a, b in cc.PAIRS:
                res = result_buffer(r0, dev, 0, b)
                l0 = launches(lo)
                lo.mul(res, ops[mode], T(xc, dev), a, b)
                if band and mode == "N":
                    assert launches(lo) - l0 == 1, "the row-band form is one launch"
                want = oracle.gemv(r0.copy(), Mc, xc, a, b, trans=mode, flags=oracle.scalar_flags(npd, a, b))
                what = str((m, n, mode, case, a, b))
                cc.assert_gemv_expectations(want, exp, a, b, what)
                check_against_oracle(res.cpu().numpy(), want, tol=TOL_CGEMV[npd], what=what)


@pytest.mark.parametrize("npd", cc.CDTS, ids=CDT_IDS)
@pytest.mark.parametrize("m,n", cc.GEMV_SHAPES)
def test_complex_dense_gemv_nonfinite(lo, dev, npd, m, n):
    """M*x, transpose(M)*u, M'*u and conj(M)*x on complex data — (520, 260) reaches the 16-byte column form: NaN in Re(x) (all
    NaN), one Inf in Re(x) / Im(x), one NaN in Re(M) (one output, both components), one -Inf in Im(M), an entry a + 0i
    opposite the Inf in Re(x) (NaN in the imaginary part of that output ONLY — no recovery, as base/complex.jl), x scaled by
    1e120 / 1e-120 (1e15 / 1e-15); real and complex (α, β), β = 0 on NaN."""
    _run_gemv(lo, dev, npd, m, n)


@pytest.mark.parametrize("npd", cc.CDTS, ids=CDT_IDS)
def test_complex_dense_gemv_nonfinite_row_band(lo, dev, npd):
    """The same cases at the smallest shape `cgemv_rows_band` admits on this device (m = 8 * VR * num_cu, n = 1024): M*x is ONE
    launch there."""
    m, n = cc.band_shape(npd, lo.get_ctx(dev).info()["num_cu"])
    assert m * n * np.dtype(npd).itemsize <= 64 << 20
    _run_gemv(lo, dev, npd, m, n, band=True)


# =========================================================================== d. opHermitian
def _herm_dev_matrix(A, aligned, dev):
    """column-major device copy of A: on its own, or one element into a larger column-major buffer (for ComplexF32 the
    masked path: not 16-byte aligned)."""
    off = 0 if aligned else 1
    n = A.shape[0]
    big = np.full((n + off + (n + off) % 2, n), NANC, A.dtype)      # an even leading dimension: 16-byte aligned columns when off = 0
    big[off:n + off, :] = A
    bigd = T(np.ascontiguousarray(big.T), dev).t()
    return bigd[off:n + off, :]


@pytest.mark.parametrize("npd,n,d_real,aligned", cc.HERM_PARAMS,
                         ids=[f"{'c128' if p[0] == np.complex128 else 'c64'}-{p[1]}-{'dreal' if p[2] else 'dcplx'}-{'al' if p[3] else 'off1'}"
                              for p in cc.HERM_PARAMS])
def test_complex_hermitian_nonfinite_both_forms(lo, dev, npd, n, d_real, aligned):
    """mulHermitian! on complex A with a real and a complex d, in both device forms — the single-pass strip kernel and the
    two-pass form (`cherm_two_pass` = 1) — each against the oracle; n reaches the ragged body only, one diagonal block of a
    full row group plus a ragged group, and interior strips. Every element on and above the diagonal of A is NaN + NaN i and
    never surfaces; it never meets v either: one Inf in v gives ±Inf and NO NaN (an element at or above the diagonal that
    is zeroed and then multiplied by v would give 0 * Inf = NaN in rows and columns the stored triangle never touches)."""
    ctx = lo.get_ctx(dev)
    base = cc.herm_base(npd, n, d_real, seed=n + 2 * d_real)
    r0 = base[3]
    for case in cc.HERM_CASES:
        for a, b in cc.PAIRS:
            (d, A, L, v), exp = cc.herm_case(npd, base, case, a, b)
            want = oracle.hermitian_mul(r0.copy(), d, L, v, a, b, flags=oracle.scalar_flags(npd, a, b))
            cc.assert_expectations(want, exp, str((n, case, a, b)))
            H = lo.opHermitian(T(d, dev), _herm_dev_matrix(A, aligned, dev))
            for two_pass in (0, 1):
                with ctx.tuned(cherm_two_pass=two_pass):
                    res = result_buffer(r0, dev, 0, b)
                    lo.mul(res, H, T(v, dev), a, b)
                check_against_oracle(res.cpu().numpy(), want, tol=TOL_CHERM[npd],
                                     what=str(("two-pass" if two_pass else "strip", n, d_real, aligned, case, a, b)))
    ctx.sync()


# =========================================================================== e. sparse
@pytest.mark.parametrize("npd", cc.CDTS, ids=CDT_IDS)
@pytest.mark.parametrize("layout", ["csc", "csr"])
def test_complex_sparse_nonfinite(lo, dev, npd, layout):
    """A*x, transpose(A)*u and A'*u of a complex SparseMatrixCSC, handed over as CSC and as the CSR storage of the same matrix;
    one column and one row are longer than a chunk. NaN / Inf in Re or Im of the vector reach only the outputs that store
    an entry opposite; a stored 0 + 0i opposite the Inf gives NaN in both components there and nowhere else, a stored
    a + 0i gives NaN in one component there; an Inf in a stored value. (The real-planes form behind
    MXLO_SPARSE_COMPLEX_PLANES=1 is out of scope: see the module docstring.)"""
    S = cc.sparse_matrix(npd)
    m, n, colptr, rowval = S["m"], S["n"], S["colptr"], S["rowval"]
    rng = np.random.default_rng(10)
    xs = {False: cc.cunit_mags(rng, n, npd), True: cc.cunit_mags(rng, m, npd)}

    def device_op(nz):
        M = torch.sparse_csc_tensor(torch.from_numpy(colptr), torch.from_numpy(rowval), torch.from_numpy(nz), size=(m, n)).to(dev)
        if layout == "csr":
            M = M.to_sparse_csr()
            assert M.values().numel() == nz.size, "the explicit stored zeros must survive the layout change"
        return lo.LinearOperatorFromMatrix(M)

    base_op = device_op(S["nz"])
    for mode in cc.SPARSE_MODES:
        trans = mode != "N"
        nout = n if trans else m
        r0 = cc.cunit_mags(rng, nout, npd)
        for case in cc.SPARSE_CASES:
            (nz, xc), exp = cc.sparse_case(npd, S, xs[trans], mode, case)
            Sp = device_op(nz) if case == "inf_nz" else base_op
            op = {"N": Sp, "T": lo.transpose(Sp), "C": lo.adjoint(Sp)}[mode]
            scale = cc.sparse_scale(S, nz, xc, mode)
            counts = {}
            for a, b in cc.PAIRS:
                res = result_buffer(r0, dev, 0, b)
                xd = T(xc, dev)
                l0 = launches(lo)
                lo.mul(res, op, xd, a, b)
                counts[cc.real_pair(a, b)] = launches(lo) - l0
                want = oracle.csc_mul(r0.copy(), colptr + 1, rowval + 1, nz, m, n, xc, a, b, trans=False if mode == "N" else mode,
                                      flags=oracle.scalar_flags(npd, a, b))
                what = str((layout, mode, case, a, b))
                cc.assert_expectations(want, exp, what)
                if "nan_at_real_pair" in exp and cc.real_pair(a, b):
                    assert np.array_equal(np.flatnonzero(np.isnan(cc.rview(want))), exp["nan_at_real_pair"]), what
                check_against_oracle(res.cpu().numpy(), want, what=what,
                                     atol=TOL_CSPARSE[npd] * (abs(a) * scale + abs(b) * float(np.abs(r0).max())))
            if layout == "csc":          # a Complex α is applied inside the sweep (x scaled at the gather in mode N): no extra pass
                assert counts[False] == counts[True], (mode, case, counts)


# =========================================================================== f. real operators on complex vectors
def _real_family(lo, dev, family, rd, rng):
    """(device operator, n_in, n_out, plane oracle: real vector -> real vector, tolerance kwargs for (a, b, x))."""
    z = lambda k: np.empty(k, rd)
    f0 = oracle.scalar_flags(rd, 1.0, 0.0)
    if family in ("dense", "dense_T"):
        m, n = 70, 53
        M = unit_mags(rng, (m, n), rd)
        op = lo.LinearOperatorFromMatrix(TM(M, dev))
        tr = family == "dense_T"
        nin, nout = (m, n) if tr else (n, m)
        return (op.T if tr else op), nin, nout, (lambda x: oracle.gemv(z(nout), M, x, 1.0, 0.0, trans=tr, flags=f0)), dict(tol=TOL_GEMV[rd])
    if family == "hermitian":
        n = 129
        A = unit_mags(rng, (n, n), rd)
        A[np.triu_indices(n)] = np.nan
        d = unit_mags(rng, n, rd)
        op = lo.opHermitian(T(d, dev), TM(A, dev))
        return op, n, n, (lambda x: oracle.hermitian_mul(z(n), d, np.tril(A, -1), x, 1.0, 0.0, flags=f0)), dict(tol=TOL_HERM[rd])
    if family == "sparse":
        m, n = 300, 200
        dense = unit_mags(rng, (m, n), rd) * (rng.random((m, n)) < 0.05)
        dense[:, 9] = unit_mags(rng, m, rd)
        cols = [np.flatnonzero(dense[:, c]) for c in range(n)]
        colptr = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int64)
        rowval = np.concatenate(cols).astype(np.int64)
        nz = np.concatenate([dense[c_, i_] for i_, c_ in enumerate(cols)]).astype(rd)
        op = lo.LinearOperatorFromMatrix(lo.sparse_csc(colptr, rowval, nz, m, n, index_base=0, device=dev))
        absD = np.abs(dense.astype(np.float64))
        plane = lambda x: oracle.csc_mul(z(m), colptr + 1, rowval + 1, nz, m, n, x, 1.0, 0.0, flags=f0)
        return op, n, m, plane, dict(sparse_abs=absD)
    if family == "kron":
        A, B = unit_mags(rng, (6, 5), rd), unit_mags(rng, (7, 9), rd)
        op = lo.kron(TM(A, dev), TM(B, dev))
        return op, 45, 42, (lambda x: oracle.kron_mul(z(42), A, B, x, 1.0, 0.0, flags=f0)), dict(tol=TOL_KRON[rd])
    sizes = (37, 101, 63)
    Ms = [unit_mags(rng, (k, k), rd) for k in (sizes[0], sizes[2])]
    dmid = unit_mags(rng, sizes[1], rd)
    op = lo.BlockDiagonalOperator(lo.LinearOperatorFromMatrix(TM(Ms[0], dev)), lo.opDiagonal(T(dmid, dev)),
                                  lo.LinearOperatorFromMatrix(TM(Ms[1], dev)))
    s1, s2, ntot = sizes[0], sizes[0] + sizes[1], sum(sizes)

    def plane(x):
        return np.concatenate([oracle.gemv(z(sizes[0]), Ms[0], x[:s1].copy(), 1.0, 0.0, flags=f0),
                               oracle.diag_mul(z(sizes[1]), dmid, x[s1:s2].copy(), 1.0, 0.0, flags=f0),
                               oracle.gemv(z(sizes[2]), Ms[1], x[s2:].copy(), 1.0, 0.0, flags=f0)])
    return op, ntot, ntot, plane, dict(tol=TOL_GEMV[rd])


@pytest.mark.parametrize("npd", cc.CDTS, ids=CDT_IDS)
@pytest.mark.parametrize("family", cc.REAL_ON_COMPLEX)
def test_real_operator_on_complex_vector_keeps_the_planes_apart(lo, dev, npd, family):
    """A real operator applied to the two planes of a complex vector (operators.py: _mul_real_op_complex_vec): an Inf or a NaN
    in Re(v) only leaves the imaginary plane of the result bit-identical to the clean apply's (real α, β), and the other way
    round; the whole result has the class map of the family's REAL oracle run on each plane and joined as
    α*(yr + i*yi) + β*res by the oracle's complex eye_mul, within the family's real tolerance on the finite positions."""
    rd = cc.RD[npd]
    rng = np.random.default_rng(123)
    op, nin, nout, plane, tolkw = _real_family(lo, dev, family, rd, rng)
    v = cc.cunit_mags(rng, nin, npd)
    r0 = cc.cunit_mags(rng, nout, npd)

    def run(x, a, b):
        res = result_buffer(r0, dev, 0, b)
        lo.mul(res, op, T(x, dev), a, b)
        return res.cpu().numpy()

    for a, b in cc.PAIRS:
        clean = run(v, a, b)
        for which, val in cc.PLANE_POISONS:
            x = v.copy()
            pos = nin // 2 + 1
            x[pos] = complex(val, x[pos].imag) if which == "re" else complex(x[pos].real, val)
            got = run(x, a, b)
            what = str((family, which, val, a, b))
            y = np.empty(nout, npd)
            y.real, y.imag = plane(np.ascontiguousarray(x.real)), plane(np.ascontiguousarray(x.imag))
            want = oracle.eye_mul(r0.copy(), y, a, b, flags=oracle.scalar_flags(npd, a, b) | oracle.TAIL_BETA)
            assert not np.isfinite(cc.rview(want)).all(), what
            if "sparse_abs" in tolkw:                    # the bound of test_gpu_sparse.py, |x| the modulus of the complex entries
                xa = np.where(np.isfinite(x), np.abs(x.astype(np.complex128)), 0.0)
                kw = dict(atol=TOL_SPARSE[rd] * (abs(a) * float((tolkw["sparse_abs"] @ xa).max()) + abs(b) * float(np.abs(r0).max())))
            else:
                kw = tolkw
            check_against_oracle(got, want, what=what, **kw)
            if cc.real_pair(a, b):
                other = (lambda z: z.imag) if which == "re" else (lambda z: z.real)
                assert np.array_equal(np.ascontiguousarray(other(got)).view(np.uint8), np.ascontiguousarray(other(clean)).view(np.uint8)), \
                    what + ": the untouched plane changed"
    lo.get_ctx(dev).sync()


# =========================================================================== g. wrapper routing
@pytest.mark.parametrize("npd", cc.CDTS, ids=CDT_IDS)
def test_conj_sandwich_routing_nonfinite(lo, dev, npd):
    """A complex operator that has tprod! only: its adjoint is conj!(res); tprod!(res, conj.(v), conj(α), conj(β)); conj!(res)
    (operators.py: _call_conj_sandwich, src/adjtrans.jl:127-136); one with ctprod! only: its transpose likewise
    (:193-204). On a vector with -0.0 imaginary parts and one NaN, and on one with an Inf, the result has the class map of
    the oracle's gemv in mode C (resp. T) and is within the GEMV tolerance elsewhere."""
    dtype = TD[npd]
    rng = np.random.default_rng(5)
    m, n = 37, 23
    M = cc.cunit_mags(rng, (m, n), npd)
    dense = lo.LinearOperatorFromMatrix(TM(M, dev))
    S = lo.Storage(dtype, dev)
    prod = lambda r, v, a, b: lo.mul(r, dense, v, a, b)
    only_t = lo.LinearOperator(dtype, m, n, False, False, prod, lambda r, v, a, b: lo.mul(r, dense.T, v, a, b), None, S=S)
    only_ct = lo.LinearOperator(dtype, m, n, False, False, prod, None, lambda r, v, a, b: lo.mul(r, dense.H, v, a, b), S=S)
    r0 = cc.cunit_mags(rng, n, npd)
    for op, mode in ((only_t.H, "C"), (only_ct.T, "T")):
        for val in (np.nan, np.inf):
            u = np.empty(m, npd)
            u.real, u.imag = unit_mags(rng, m, cc.RD[npd]), -0.0
            u[m // 2] = complex(val, -0.0)
            assert np.signbit(u.imag).all()
            for a, b in cc.PAIRS:
                res = result_buffer(r0, dev, 0, b)
                lo.mul(res, op, T(u, dev), a, b)
                want = oracle.gemv(r0.copy(), M, u, a, b, trans=mode, flags=oracle.scalar_flags(npd, a, b))
                assert not np.isfinite(cc.rview(want)).any()
                check_against_oracle(res.cpu().numpy(), want, tol=TOL_CGEMV[npd], what=str((mode, val, a, b)))
    assert (only_t.ntprod, only_t.nctprod, only_ct.nctprod, only_ct.ntprod) == (6, 0, 6, 0)    # the sandwiches ran, not a direct closure
