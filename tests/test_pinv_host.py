"""CPU: the host half of opPinv(A, rtol=...) — the export and the signature, the rtol checks that run before A is looked at
and their place in front of opQR's refusals, the three C-ABI declarations, and the launch counts an apply promises. No
device call anywhere in this file."""
import inspect

import pytest
import torch

ENTRY_POINTS = ("mxlo_cod_factor", "mxlo_pinv_mul", "mxlo_pinv_mul_block")


def cpu_matrix():
    return torch.ones((5, 3), dtype=torch.float64)


def test_opPinv_is_exported_with_its_signature(lo):
    assert lo.opPinv is lo.linalg.opPinv
    ps = inspect.signature(lo.opPinv).parameters
    assert list(ps) == ["A", "rtol"]
    assert ps["rtol"].default is None


@pytest.mark.parametrize("rtol", [-1e-3, 1.0, 2.0, float("nan")])
def test_rtol_outside_its_range_is_a_value_error(lo, rtol):
    with pytest.raises(ValueError, match="rtol"):
        lo.opPinv(cpu_matrix(), rtol=rtol)


@pytest.mark.parametrize("rtol", ["x", True, 1j])
def test_rtol_must_be_a_real_number(lo, rtol):
    with pytest.raises(TypeError, match="rtol"):
        lo.opPinv(cpu_matrix(), rtol=rtol)


def test_the_rtol_checks_run_before_A_is_looked_at(lo):
    """not even the type of A is seen before them"""
    with pytest.raises(ValueError, match="rtol"):
        lo.opPinv(None, rtol=2.0)
    with pytest.raises(TypeError, match="rtol"):
        lo.opPinv(None, rtol="x")


def test_the_refusals_of_opQR_follow_in_their_order(lo):
    with pytest.raises(TypeError):
        lo.opPinv(torch.ones(4, dtype=torch.float64))
    with pytest.raises(TypeError):
        lo.opPinv(None)
    with pytest.raises(lo.LinearOperatorException):
        lo.opPinv(torch.ones((0, 3), dtype=torch.complex128))               # empty is refused before the element type
    with pytest.raises(TypeError, match="real Float64 / Float32 only"):
        lo.opPinv(torch.ones((5, 3), dtype=torch.complex128), rtol=1e-8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lo.opPinv(cpu_matrix())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lo.opPinv(cpu_matrix(), rtol=0.0)


def test_header_declarations_prototypes_and_exports(lo):
    syms = lo._lib.header_symbols()
    L = lo._lib.lib()
    for name in ENTRY_POINTS:
        assert name in syms and name in lo._lib._PROTOS, name
        assert hasattr(L, name), name                       # exported by the built library


def test_launch_counts_of_an_apply(lo):
    la = lo.linalg
    assert list(inspect.signature(la.pinv_launches).parameters) == ["rank", "nf"]
    assert list(inspect.signature(la.pinv_block_launches).parameters) == ["rank", "nf", "k"]
    for r in (1, 63, 64, 65, 129):
        nb = -(-r // 64)
        assert la.pinv_launches(r, r) == la.qrp_launches(r)                 # full rank: the pivoted operator
        for nf in (r + 1, r + 64, 4 * r + 5):
            got = la.pinv_launches(r, nf)
            assert isinstance(got, int) and got == 3 * nb + 2, (r, nf, got)
        for k in (1, 7, 8, 9, 17):
            assert la.pinv_block_launches(r, r + 1, k) == -(-k // 8) * (3 * nb + 2), (r, k)
            assert la.pinv_block_launches(r, r, k) == la.qrp_block_launches(r, k), (r, k)


def test_opQR_points_to_opPinv(lo):
    assert "opPinv" in lo.opQR.__doc__
