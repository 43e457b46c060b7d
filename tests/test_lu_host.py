"""CPU: the host half of opLU (the general dense `M \\ v` of src/linalg.jl:27-32) — the public names, the C-ABI declarations
they rest on, and the refusals that happen before any device work. No device call anywhere in this file."""
import pytest
import torch

ENTRY_POINTS = ("mxlo_getrf", "mxlo_lu_mul")


def test_public_names_header_declarations_and_exports(lo):
    assert callable(lo.opLU)
    assert issubclass(lo.SingularException, Exception) and lo.SingularException(3).info == 3
    assert "3" in str(lo.SingularException(3))
    syms = lo._lib.header_symbols()
    L = lo._lib.lib()
    for name in ENTRY_POINTS:
        assert name in syms and name in lo._lib._PROTOS, name
        assert hasattr(L, name), name                       # exported by the built library
    # mxlo_potrf's arguments without m_rowmajor, with a second set of block inverses and the permutation
    assert len(lo._lib._PROTOS["mxlo_getrf"]) == len(lo._lib._PROTOS["mxlo_potrf"]) + 1
    # mxlo_chol_mul's with the second set of block inverses, the permutation and op_mode
    assert len(lo._lib._PROTOS["mxlo_lu_mul"]) == len(lo._lib._PROTOS["mxlo_chol_mul"]) + 3


def test_non_square_is_a_shape_mismatch_before_any_device_work(lo):
    """CPU tensors: the check fires before the device is looked at."""
    for shape in ((3, 5), (5, 3)):
        with pytest.raises(lo.LinearOperatorException, match="shape mismatch"):
            lo.opLU(torch.ones(shape, dtype=torch.float64))
    with pytest.raises(lo.LinearOperatorException, match="shape mismatch"):       # before the element type
        lo.opLU(torch.ones((3, 5), dtype=torch.complex128))


def test_complex_and_half_element_types_are_a_stated_limit(lo):
    for dt in (torch.complex128, torch.complex64):
        with pytest.raises(TypeError, match="real Float64 / Float32 only"):
            lo.opLU(torch.eye(4, dtype=dt))
    with pytest.raises(TypeError):
        lo.opLU(torch.eye(4, dtype=torch.float16))
    with pytest.raises(TypeError):
        lo.opLU([[1.0, 0.0], [0.0, 1.0]])


def test_a_host_matrix_is_refused_loudly(lo):
    for flags in ({}, {"symm": True, "herm": True}):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            lo.opLU(torch.eye(4, dtype=torch.float64), **flags)
