"""CPU: the host half of opLDL (ext/LinearOperatorsLDLFactorizationsExt.jl:5-18) — the public names, the C-ABI declarations
they rest on, and the refusals that happen before any device work. No device call anywhere in this file."""
import pytest
import torch

ENTRY_POINTS = ("mxlo_ldlt", "mxlo_ldl_mul")


def test_public_names_header_declarations_and_exports(lo):
    assert callable(lo.opLDL)
    assert issubclass(lo.ZeroPivotException, Exception) and lo.ZeroPivotException(71).info == 71
    assert "71" in str(lo.ZeroPivotException(71))
    syms = lo._lib.header_symbols()
    L = lo._lib.lib()
    for name in ENTRY_POINTS:
        assert name in syms and name in lo._lib._PROTOS, name
        assert hasattr(L, name), name                       # exported by the built library
    assert len(lo._lib._PROTOS["mxlo_ldlt"]) == len(lo._lib._PROTOS["mxlo_potrf"]) + 1        # the pivots d
    assert len(lo._lib._PROTOS["mxlo_ldl_mul"]) == len(lo._lib._PROTOS["mxlo_chol_mul"]) + 1


def test_non_square_is_a_shape_mismatch_before_any_device_work(lo):
    """ext/LinearOperatorsLDLFactorizationsExt.jl:7 — CPU tensors: the check fires before the device is looked at."""
    for shape in ((3, 5), (5, 3)):
        for check in (False, True):
            with pytest.raises(lo.LinearOperatorException, match="shape mismatch"):
                lo.opLDL(torch.ones(shape, dtype=torch.float64), check=check)


def test_complex_and_half_element_types_are_a_stated_limit(lo):
    for dt in (torch.complex128, torch.complex64):
        with pytest.raises(TypeError, match="real Float64 / Float32 only"):
            lo.opLDL(torch.eye(4, dtype=dt))
    with pytest.raises(TypeError):
        lo.opLDL(torch.eye(4, dtype=torch.float16))
    with pytest.raises(TypeError):
        lo.opLDL([[1.0, 0.0], [0.0, 1.0]])


def test_a_host_matrix_is_refused_loudly(lo):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lo.opLDL(torch.eye(4, dtype=torch.float64))
