"""CPU checks of complex_nonfinite_cases.py, the generators behind test_gpu_complex_nonfinite.py: every generator satisfies the
input rules for every parametrisation the device file uses (the lists are imported, not copied), the oracle's class maps
are the ones the cases are built to have (which also protects the cases against an oracle change), the pattern of the
elementwise leaves tells a Real scalar from its Complex(x, 0) spelling, and a NumPy model of the `0 * Inf` defect of a
select-then-multiply diagonal tile has ANOTHER class map than the oracle on the opHermitian cases — the cases discriminate."""
import numpy as np
import pytest

import oracle
import complex_nonfinite_cases as cc
from test_gpu_nonfinite import special_values

CDT_IDS = ["c128", "c64"]


@pytest.mark.parametrize("npd", cc.CDTS, ids=CDT_IDS)
def test_cpattern_meets_every_pair_of_values(npd):
    sv = special_values(cc.RD[npd])
    key = lambda a: np.searchsorted(np.sort(sv.view({8: np.uint64, 4: np.uint32}[sv.itemsize])),
                                    np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32}[sv.itemsize]))
    for which in range(3):
        for shift in (0, 1, 7):
            z = cc.cpattern(npd, 4099, which, shift)
            pairs = set(zip(key(z.real).tolist(), key(z.imag).tolist()))
            assert len(pairs) == sv.size ** 2, (which, shift, len(pairs))
    # the three operands of a leaf meet in every pair of values too (real parts of d and v, real of d and imaginary of v)
    d, v = cc.cpattern(npd, 4099, 0, 0), cc.cpattern(npd, 4099, 1, 0)
    assert len(set(zip(key(d.real).tolist(), key(v.real).tolist()))) == sv.size ** 2
    assert len(set(zip(key(d.real).tolist(), key(v.imag).tolist()))) == sv.size ** 2
    for n in cc.LEAF_SIZES:
        assert cc.cpattern(npd, n, 2, 3).shape == (n,) and cc.cpattern(npd, n, 2, 3).dtype == npd


@pytest.mark.parametrize("npd", cc.CDTS, ids=CDT_IDS)
def test_scalar_variants_cover_every_alpha_with_every_beta_class(npd):
    var = cc.scalar_variants(npd)
    py = [(a, b) for a, b in var if not isinstance(a, (np.floating, np.complexfloating))]
    assert len(py) == 3 * (len(cc.REAL_ALPHAS) + len(cc.COMPLEX_ALPHAS))
    for a in cc.REAL_ALPHAS + cc.COMPLEX_ALPHAS:
        mine = [b for x, b in py if type(x) is type(a) and x == a and np.signbit(complex(x).real) == np.signbit(complex(a).real)
                and np.signbit(complex(x).imag) == np.signbit(complex(a).imag)]
        assert len(mine) == 3, a
        assert sum(cc.is_zero(b) for b in mine) == 1
        assert sum(not cc.is_zero(b) and not isinstance(b, complex) for b in mine) == 1
        assert sum(not cc.is_zero(b) and isinstance(b, complex) for b in mine) == 1
    if npd == np.complex64:
        n32 = [(a, b) for a, b in var if isinstance(a, (np.float32, np.complex64))]
        assert len(n32) == len(py) and all(isinstance(b, (np.float32, np.complex64)) for _, b in n32)
        assert {oracle.scalar_flags(npd, a, b) & oracle.SCALARS_F64 for a, b in n32} == {0}
        assert {oracle.scalar_flags(npd, a, b) & oracle.SCALARS_F64 for a, b in py} == {oracle.SCALARS_F64}
    else:
        assert len(var) == len(py)


@pytest.mark.parametrize("npd", cc.CDTS, ids=CDT_IDS)
def test_real_and_complex_spelling_of_a_scalar_differ_on_the_pattern(npd):
    assert cc.scalar_spellings_differ(npd) == (True, True)


@pytest.mark.parametrize("npd", cc.CDTS, ids=CDT_IDS)
def test_cunit_mags_has_no_zero_component_and_unit_magnitudes(npd):
    z = cc.rview(cc.cunit_mags(np.random.default_rng(0), (50, 40), npd))
    assert z.dtype == cc.RD[npd] and (np.abs(z) >= 0.5).all() and (np.abs(z) <= 1.0).all()
    assert (z > 0).any() and (z < 0).any()


@pytest.mark.parametrize("npd", cc.CDTS, ids=CDT_IDS)
def test_householder_cases_keep_the_rules_and_the_oracle_agrees(npd):
    rng = np.random.default_rng(77)
    for n in cc.HOUSE_SIZES:
        for case in cc.HOUSE_CASES:
            for p in (5, n - 1):
                (h, v), exp = cc.house_case(npd, n, case, p, rng)                   # asserts the rules itself
                r0 = cc.cunit_mags(rng, n, npd)
                for a, b in cc.PAIRS:
                    want = oracle.householder_mul(r0.copy(), h, v, a, b, flags=oracle.scalar_flags(npd, a, b))
                    cc.assert_expectations(want, exp, str((n, case, p, a, b)))
                    if case in ("inf_re_v", "inf_im_v"):
                        assert not np.isfinite(cc.rview(want)).any()


@pytest.mark.parametrize("npd", cc.CDTS, ids=CDT_IDS)
@pytest.mark.parametrize("m,n", cc.GEMV_SHAPES)
def test_gemv_cases_keep_the_rules_and_the_oracle_agrees(npd, m, n):
    rng = np.random.default_rng(m * 7 + n)
    M = cc.cunit_mags(rng, (m, n), npd)
    xs = {True: cc.cunit_mags(rng, n, npd), False: cc.cunit_mags(rng, m, npd)}
    for case in cc.GEMV_CASES:
        for mode in cc.GEMV_MODES:
            rows = mode in ("N", "J")
            (Mc, xc), exp = cc.gemv_case(npd, M, xs[rows], mode, case)
            r0 = cc.cunit_mags(rng, m if rows else n, npd)
            for a, b in cc.PAIRS:
                want = oracle.gemv(r0.copy(), Mc, xc, a, b, trans=mode, flags=oracle.scalar_flags(npd, a, b))
                cc.assert_gemv_expectations(want, exp, a, b, str((m, n, mode, case, a, b)))
                if case in ("inf_re_x", "inf_im_x") and cc.real_pair(a, b):
                    w = cc.rview(want)
                    assert np.isinf(w).all(), "one Inf per reduction, no zero opposite it: ±Inf everywhere, no NaN"


def test_band_shape_follows_the_kernel_rule():
    assert cc.band_shape(np.complex128, 256) == (2048, 1024) and cc.band_shape(np.complex64, 256) == (4096, 1024)
    for npd in cc.CDTS:
        m, n = cc.band_shape(npd, 304)
        assert m * n * np.dtype(npd).itemsize <= 64 << 20


@pytest.mark.parametrize("npd,n,d_real,aligned", [p for p in cc.HERM_PARAMS if p[3]],
                         ids=[f"{'c128' if p[0] == np.complex128 else 'c64'}-{p[1]}-{'dreal' if p[2] else 'dcplx'}" for p in cc.HERM_PARAMS if p[3]])
def test_hermitian_cases_the_oracle_agrees_and_the_defect_model_does_not(npd, n, d_real, aligned):
    """The oracle's expectations of the device test hold; and for the `inf_v` / `nan_v` cases the dense model of the defect
    (zeroed elements still multiplied by v) has another class map, so a kernel with the defect fails those cases."""
    base = cc.herm_base(npd, n, d_real, seed=n + 2 * d_real)
    r0 = base[3]
    assert np.isnan(cc.rview(base[1][np.triu_indices(n)])).all()
    for case in cc.HERM_CASES:
        for a, b in cc.PAIRS:
            (d, A, L, v), exp = cc.herm_case(npd, base, case, a, b)
            if cc.real_pair(a, b) and case != "big_v":
                assert exp, "every non-finite case fixes a class map for real scalars"
            want = oracle.hermitian_mul(r0.copy(), d, L, v, a, b, flags=oracle.scalar_flags(npd, a, b))
            what = str((n, d_real, case, a, b))
            cc.assert_expectations(want, exp, what)
            full = oracle.hermitian_mul(r0.copy(), d, np.where(np.isnan(A), 0, A), v, a, b, flags=oracle.scalar_flags(npd, a, b))
            assert np.array_equal(cc.class_map(full), cc.class_map(want)), "the oracle reads the strict lower triangle only"
            # (nan_v with a complex d or complex scalars is all NaN in the oracle already: nothing left to tell apart)
            if case in ("inf_re_v", "ninf_im_v") or (case == "nan_v" and d_real and cc.real_pair(a, b)):
                model = cc.defect_model(d, L, v, a, b, r0)
                assert not np.array_equal(cc.class_map(model), cc.class_map(want)), what + ": the defect would go unseen"
            elif case == "big_v":
                model = cc.defect_model(d, L, v, a, b, r0)              # on finite data the model IS the operator
                assert np.allclose(model, want.astype(np.complex128), rtol=1e-4 if npd == np.complex64 else 1e-11, atol=0)


@pytest.mark.parametrize("npd", cc.CDTS, ids=CDT_IDS)
def test_sparse_cases_keep_the_rules_and_the_oracle_agrees(npd):
    S = cc.sparse_matrix(npd)
    m, n, colptr, rowval = S["m"], S["n"], S["colptr"], S["rowval"]
    assert np.diff(colptr).max() == 3000 > 2048 and int((rowval == S["long_row"]).sum()) >= 2594 > 2048   # a chunk is 2048
    rng = np.random.default_rng(10)
    xs = {False: cc.cunit_mags(rng, n, npd), True: cc.cunit_mags(rng, m, npd)}
    for mode in cc.SPARSE_MODES:
        trans = mode != "N"
        r0 = cc.cunit_mags(rng, n if trans else m, npd)
        for case in cc.SPARSE_CASES:
            (nz, xc), exp = cc.sparse_case(npd, S, xs[trans], mode, case)
            assert cc.sparse_scale(S, nz, xc, mode) > 0
            for a, b in cc.PAIRS:
                want = oracle.csc_mul(r0.copy(), colptr + 1, rowval + 1, nz, m, n, xc, a, b, trans=False if mode == "N" else mode,
                                      flags=oracle.scalar_flags(npd, a, b))
                what = str((mode, case, a, b))
                cc.assert_expectations(want, exp, what)
                assert not np.isfinite(cc.rview(want)).all(), what
                if "nan_at_real_pair" in exp and cc.real_pair(a, b):
                    assert np.array_equal(np.flatnonzero(np.isnan(cc.rview(want))), exp["nan_at_real_pair"]), what
