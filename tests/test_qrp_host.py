"""CPU: the host half of opQR(A, pivot=True, rtol=...) — the signature, the argument checks that run before A is looked at
and their place in front of the existing refusals, the three C-ABI declarations, and the launch counts the pivoted apply
promises. No device call anywhere in this file."""
import inspect

import pytest
import torch

ENTRY_POINTS = ("mxlo_geqp3", "mxlo_qrp_mul", "mxlo_qrp_mul_block")


def cpu_matrix():
    return torch.ones((5, 3), dtype=torch.float64)


def test_signature_of_opQR(lo):
    ps = inspect.signature(lo.opQR).parameters
    assert list(ps) == ["A", "pivot", "rtol"]
    assert ps["pivot"].default is False and ps["rtol"].default is None


@pytest.mark.parametrize("pivot", [1, "yes"])
def test_pivot_must_be_a_bool(lo, pivot):
    with pytest.raises(TypeError, match="pivot"):
        lo.opQR(cpu_matrix(), pivot=pivot)


@pytest.mark.parametrize("rtol", [-1e-3, 1.0, float("nan")])
def test_rtol_outside_its_range_is_a_value_error(lo, rtol):
    with pytest.raises(ValueError, match="rtol"):
        lo.opQR(cpu_matrix(), pivot=True, rtol=rtol)


def test_rtol_must_be_a_real_number(lo):
    with pytest.raises(TypeError, match="rtol"):
        lo.opQR(cpu_matrix(), pivot=True, rtol="x")


def test_rtol_without_pivot_is_a_value_error(lo):
    with pytest.raises(ValueError, match="pivot"):
        lo.opQR(cpu_matrix(), rtol=1e-8)
    with pytest.raises(ValueError, match="pivot"):
        lo.opQR(cpu_matrix(), pivot=False, rtol=1e-8)


def test_the_new_checks_run_before_A_is_looked_at(lo):
    """not even the type of A is seen before them"""
    with pytest.raises(TypeError, match="pivot"):
        lo.opQR(None, pivot=1)
    with pytest.raises(ValueError, match="rtol"):
        lo.opQR(None, pivot=True, rtol=2.0)


def test_the_existing_refusals_follow_in_their_order(lo):
    with pytest.raises(TypeError):
        lo.opQR(torch.ones(4, dtype=torch.float64), pivot=True)
    with pytest.raises(lo.LinearOperatorException):
        lo.opQR(torch.ones((0, 3), dtype=torch.complex128), pivot=True)
    with pytest.raises(TypeError, match="real Float64 / Float32 only"):
        lo.opQR(torch.ones((5, 3), dtype=torch.complex128), pivot=True, rtol=1e-8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lo.opQR(cpu_matrix(), pivot=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lo.opQR(cpu_matrix(), pivot=True, rtol=0.0)


def test_header_declarations_prototypes_and_exports(lo):
    syms = lo._lib.header_symbols()
    L = lo._lib.lib()
    for name in ENTRY_POINTS:
        assert name in syms and name in lo._lib._PROTOS, name
        assert hasattr(L, name), name                       # exported by the built library


def test_launch_counts_of_the_pivoted_apply(lo):
    la = lo.linalg
    assert list(inspect.signature(la.qrp_launches).parameters) == ["rank"]
    assert list(inspect.signature(la.qrp_block_launches).parameters) == ["rank", "k"]
    for r in (1, 63, 64, 65, 129):
        got = la.qrp_launches(r)
        assert isinstance(got, int) and 1 <= got <= la.qr_launches(r) + 1, (r, got)
        for k in (1, 7, 8, 9, 17):
            assert la.qrp_block_launches(r, k) == -(-k // 8) * got, (r, k)
