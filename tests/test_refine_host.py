"""CPU: the host half of `refine=r` (iterative refinement of opCholesky, opLDL, opLU) — the keyword's refusals, the
declarations, and a NumPy model of the scheme on exactly the matrices, step counts and bounds of test_gpu_refine.py
(refine_cases.py holds them). No device call anywhere in this file.

The model factors and solves in the operator's precision, keeps the residual and x in Float64 and rounds once. It shows
two things the device test relies on: the bounds are attainable by the scheme itself, and the hard LDL' inputs are hard —
the plain Float64 solve misses the bound on every one of them with more than one block of pivots."""
import numpy as np
import pytest
import torch

import refine_cases as rc

CONSTRUCTORS = ["opCholesky", "opLDL", "opLU"]


@pytest.mark.parametrize("name", CONSTRUCTORS)
def test_refine_is_checked_before_the_matrix_is_looked_at(lo, name):
    make = getattr(lo, name)
    M = torch.eye(3, dtype=torch.float64)                   # a CPU tensor: no constructor gets past its device check
    for bad in (-1, lo.linalg.MAX_REFINE + 1):
        with pytest.raises(ValueError, match="refine"):
            make(M, refine=bad)
    for bad in (1.0, True):
        with pytest.raises(TypeError, match="refine"):
            make(M, refine=bad)
    for good in (0, 1, lo.linalg.MAX_REFINE):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            make(M, refine=good)
    with pytest.raises(TypeError, match="refine"):
        make("not a tensor", refine=2.5)                    # before M is looked at at all


def test_the_new_names_are_declared_prototyped_and_exported(lo):
    syms = lo._lib.header_symbols()
    L = lo._lib.lib()
    for name in ("mxlo_chol_mul_refine", "mxlo_ldl_mul_refine", "mxlo_lu_mul_refine", "mxlo_sym_residual", "mxlo_gen_residual",
                 "mxlo_sym_snapshot", "mxlo_lu_snapshot"):
        assert name in syms, name
        assert name in lo._lib._PROTOS, name
        assert hasattr(L, name), name
    assert lo.linalg.MAX_REFINE == 8
    assert isinstance(lo.linalg.RESIDUAL_LAUNCHES, int) and lo.linalg.RESIDUAL_LAUNCHES >= 1


def test_the_block_refine_prototypes_extend_the_block_ones(lo):
    """res, ldr, ..., V, ldv, k, steps, [op_mode,] alpha, beta: the block prototype with the snapshot operands before
    `work` and `steps` after k"""
    P, i32, i64, vp = lo._lib._PROTOS, lo._lib._i32, lo._lib._i64, lo._lib._vp
    for name, extra in (("chol", [vp]), ("ldl", [vp]), ("lu", [vp, i64])):
        blk, ref = list(P[f"mxlo_{name}_mul_block"]), list(P[f"mxlo_{name}_mul_refine"])
        tail = 3 if name == "lu" else 2                     # [op_mode,] alpha, beta
        iw = len(blk) - tail - 4                            # work, V, ldv, k
        assert ref == blk[:iw] + extra + blk[iw:len(blk) - tail] + [i32] + blk[len(blk) - tail:], name


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("n", rc.SIZES + [rc.BIG])
def test_model_hard_ldl(n):
    for npd, steps in rc.LDL_CASES:
        if n == rc.BIG and npd is not np.float64:
            continue
        K, v = rc.hard_ldl(n, npd)
        eps = float(np.finfo(npd).eps)
        solve = rc.ldl_solver(K, npd)
        eta = rc.eta2(K, rc.refine_model(K, v, solve, steps, npd), v)
        eta0 = rc.eta2(K, rc.refine_model(K, v, solve, 0, npd), v)
        print(f"hard LDL' n={n} {npd.__name__} refine={steps}: eta = {eta / (n * eps):.3g} n eps, plain {eta0 / (n * eps):.3g} n eps")
        assert eta <= n * eps, (n, npd, steps, eta / (n * eps))
        if npd is np.float64 and n > 1:                     # n == 1 has no elimination: nothing to lose
            assert eta0 > n * eps, (n, eta0 / (n * eps))    # the inputs are hard: the plain solve misses the bound


@pytest.mark.parametrize("n", rc.SIZES)
def test_model_float32_forward_error(n):
    eps = float(np.finfo(np.float32).eps)
    for kind, trans in (("spd", False), ("gen", False), ("gen", True)):
        A, v = rc.cond1e4(n, kind)
        solve = rc.chol_solver(A, np.float32) if kind == "spd" else rc.lu_solver(A, np.float32, trans)
        A = A.T if trans else A
        xs = np.linalg.solve(A, v)
        err = rc.forward_error(rc.refine_model(A, v, solve, rc.F32_STEPS, np.float32), xs)
        err0 = rc.forward_error(rc.refine_model(A, v, solve, 0, np.float32), xs)
        print(f"cond 1e4 {kind}{'-T' if trans else ''} n={n}: {err / eps:.3g} eps32 after {rc.F32_STEPS} steps, plain {err0 / eps:.3g}")
        assert err <= eps, (kind, trans, n, err / eps)


@pytest.mark.parametrize("n", rc.WELL_SIZES)
def test_model_well_conditioned_float64(n):
    eps = float(np.finfo(np.float64).eps)
    for base in ("chol", "ldl", "lu", "simple"):
        A, v = rc.well(base, n)
        solve = {"chol": rc.chol_solver, "ldl": rc.ldl_solver}.get(base, rc.lu_solver)(A, np.float64)
        eta = rc.eta_inf(A, rc.refine_model(A, v, solve, 1, np.float64), v)
        assert eta <= n * eps, (base, n, eta / (n * eps))
