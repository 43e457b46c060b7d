"""CPU: the host half of opLDL(M, pivot=True) — the public names and the C-ABI declarations they rest on, the refusals that
happen before any device work, the NumPy model of the Bunch-Kaufman strategy against LAPACK's pivots, and LAPACK itself
against the backward error bound the GPU tests assert (ldl_pivot_cases.py). No device call anywhere in this file."""
import inspect

import numpy as np
import pytest
import torch

import ldl_pivot_cases as pc

ENTRY_POINTS = ("mxlo_sytrf", "mxlo_ldlp_mul", "mxlo_ldlp_mul_block")


def test_public_names_header_declarations_and_exports(lo):
    assert callable(lo.opLDL) and callable(lo.ldl_inertia) and callable(lo.ldlp_launches)
    assert list(inspect.signature(lo.opLDL).parameters) == ["M", "check", "refine", "pivot"]
    assert inspect.signature(lo.opLDL).parameters["pivot"].default is False
    syms = lo._lib.header_symbols()
    L = lo._lib.lib()
    for name in ENTRY_POINTS:
        assert name in syms and name in lo._lib._PROTOS, name
        assert hasattr(L, name), name                       # exported by the built library
    P = lo._lib._PROTOS
    assert len(P["mxlo_sytrf"]) == len(P["mxlo_ldlt"]) + 3                  # e, perm and the panel workspace
    assert len(P["mxlo_ldlp_mul"]) == len(P["mxlo_ldl_mul"]) + 2            # e and perm
    assert len(P["mxlo_ldlp_mul_block"]) == len(P["mxlo_ldl_mul_block"]) + 2


def test_the_launch_count_depends_on_n_only_and_is_within_the_contract(lo):
    assert lo.ldlp_launches(0) == 0
    for n in (1, 63, 64, 65, 128, 129, 259, 1025, 16384):
        nb = -(-n // 64)
        assert lo.ldlp_launches(n) == 2 * nb + 1              # the contract allows at most 2 ceil(n / 64) + 1
    assert lo.linalg.ldlp_block_launches(259, 9) == 2 * lo.ldlp_launches(259)


def test_pivot_must_be_a_bool_before_m_is_looked_at(lo):
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(TypeError, match="pivot must be a bool"):
            lo.opLDL("not a matrix", pivot=bad)


def test_refine_with_pivot_is_refused_before_m_is_looked_at(lo):
    with pytest.raises(ValueError, match="refine"):
        lo.opLDL("not a matrix", refine=1, pivot=True)
    with pytest.raises(TypeError, match="refine must be an int"):
        lo.opLDL("not a matrix", refine=True, pivot=True)
    with pytest.raises(ValueError, match="MAX_REFINE"):
        lo.opLDL("not a matrix", refine=99, pivot=True)


def test_non_square_complex_and_host_matrices_are_refused_in_the_existing_order(lo):
    for shape in ((3, 5), (5, 3)):
        for check in (False, True):
            with pytest.raises(lo.LinearOperatorException, match="shape mismatch"):
                lo.opLDL(torch.ones(shape, dtype=torch.complex128), check=check, pivot=True)    # square before the element type
    for dt in (torch.complex128, torch.complex64):
        with pytest.raises(TypeError, match="real Float64 / Float32 only"):
            lo.opLDL(torch.eye(4, dtype=dt), pivot=True)
    with pytest.raises(TypeError):
        lo.opLDL(torch.eye(4, dtype=torch.float16), pivot=True)
    with pytest.raises(TypeError):
        lo.opLDL([[1.0, 0.0], [0.0, 1.0]], pivot=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lo.opLDL(torch.eye(4, dtype=torch.float64), pivot=True)


class _Fake:
    def __init__(self, d, e=None):
        self._d = torch.tensor(d, dtype=torch.float64)
        if e is not None:
            self._e = torch.tensor(e, dtype=torch.float64)


def test_ldl_inertia_counts_blocks_and_works_without_e(lo):
    assert lo.ldl_inertia(_Fake([2.0, -1.0, 0.0, 3.0])) == (2, 1, 1)                      # unpivoted: no _e
    assert lo.ldl_inertia(_Fake([0.0, 0.0, -4.0], [1.0, 0.0, 0.0])) == (1, 2, 0)            # [[0, 1], [1, 0]] and -4
    assert lo.ldl_inertia(_Fake([5.0, 1.0, 1.0], [0.0, 3.0, 0.0])) == (2, 1, 0)
    assert lo.ldl_inertia(_Fake([], [])) == (0, 0, 0)
    with pytest.raises(TypeError):
        lo.ldl_inertia(object())


@pytest.mark.parametrize("n", pc.PIVOT_NS)
def test_the_numpy_model_takes_lapacks_pivots(n):
    """The model's permutation and 2 x 2 positions are LAPACK's on the cases the GPU test compares (no ties in these matrices),
    and the model's factors reconstruct the permuted matrix."""
    M = pc.problem("indef", n, np.float64)[0]
    perm, L, d, e = pc.bunch_kaufman(M)
    lperm, ltwo = pc.lapack_pivots(M)
    assert np.array_equal(perm, lperm)
    assert set(np.nonzero(e)[0].tolist()) == ltwo
    assert sorted(perm.tolist()) == list(range(n))
    R = L @ pc.block_diag_of(d, e) @ L.T - M[np.ix_(perm, perm)]
    rhs = np.abs(L) @ np.abs(pc.block_diag_of(d, e)) @ np.abs(L).T
    assert np.linalg.norm(R) <= 3 * n * np.finfo(np.float64).eps * np.linalg.norm(rhs)


def test_the_model_sees_the_structure_the_cases_are_built_for():
    _, _, _, e = pc.bunch_kaufman(pc.problem("saddle0", 130, np.float64)[0])
    assert not e.any()                                      # interchanged 1 x 1 pivots only
    perm = pc.bunch_kaufman(pc.problem("saddle0", 130, np.float64)[0])[0]
    assert not np.array_equal(perm, np.arange(130))
    for n in (65, 130, 259):
        e = pc.bunch_kaufman(pc.problem("pairs1", n, np.float64)[0])[3]
        for b in range(64, n, 64):
            assert e[b - 1] != 0.0, (n, b)                  # a 2 x 2 pivot across every boundary between blocks of 64
    e = pc.bunch_kaufman(pc.problem("indef", 130, np.float64)[0])[3]
    assert e.any() and not e.all()
    with pytest.raises(pc.ZeroPivot) as z:
        pc.bunch_kaufman(np.diag([1.0, 0.0, 1.0]))
    assert z.value.info == 2


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=["f64", "f32"])
def test_lapack_meets_the_bound_the_gpu_tests_assert(dtype):
    """eta of sytrf / sytrs in the same precision is at most 0.87 n eps on every case and size (n >= 5: below 0.2), so
    3 n eps is a bound the reference meets."""
    eps = float(torch.finfo(dtype).eps)
    todo = pc.combos() + ([("indef", pc.N_BIG), ("pairs1", pc.N_BIG)] if dtype is torch.float64 else [])
    worst = 0.0
    for case, n in todo:
        M, v, nM, _ = pc.problem(case, n, pc.NP[dtype])
        e = pc.eta(M, nM, pc.lapack_solve(M, v, dtype), v) / (n * eps)
        worst = max(worst, e)
        assert e <= 0.87, (case, n, e)
        assert n < 5 or e <= 0.2, (case, n, e)
    print(f"LAPACK {dtype}: worst eta = {worst:.3f} n eps")


def test_the_cases_are_well_conditioned_enough_for_the_inertia_test():
    """A factorisation with backward error 3 n eps |M| has the inertia of M + dM, |dM| <= 3 n eps |M|, which is M's as long as no
    eigenvalue is that close to zero. The cases keep a factor 1000 from it; the smallest ratio min |lambda| / max |lambda| is
    4.5e-9 (saddle0 at n = 128, whose B is square), the next one 1.9e-7 (saddle0 at n = 64)."""
    eps = np.finfo(np.float64).eps
    worst = 1.0
    for case, n in pc.combos():
        w = pc.problem(case, n, np.float64)[3]
        ratio = np.abs(w).min() / np.abs(w).max()
        worst = min(worst, ratio)
        assert ratio >= 1000 * 3 * n * eps, (case, n, ratio)
    print(f"smallest min |lambda| / max |lambda|: {worst:.2e}")
