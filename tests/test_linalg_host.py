"""CPU: the host half of opCholesky / opInverse (src/linalg.jl:27-58) — the public names, the C-ABI declarations they rest
on, and the refusals that happen before any device work. No device call anywhere in this file."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mxlo_tri_kind", "mxlo_tri_prepare", "mxlo_potrf", "mxlo_trisolve_mul", "mxlo_chol_mul")


def test_public_names_and_header_declarations(lo):
    assert callable(lo.opCholesky) and callable(lo.opInverse)
    assert issubclass(lo.PosDefException, Exception) and lo.PosDefException(4).info == 4
    syms = lo._lib.header_symbols()
    for name in ENTRY_POINTS:
        assert name in syms and name in lo._lib._PROTOS, name
    with open(os.path.join(ROOT, "linearoperators.jl_amd", "csrc", "Makefile")) as f:
        assert "linalg.hip" in f.read()


def test_block_width_of_the_host_mirror_is_the_kernels(lo):
    with open(os.path.join(ROOT, "linearoperators.jl_amd", "csrc", "linalg.hip")) as f:
        assert f"constexpr int NB = {lo.linalg.BLOCK};" in f.read()


@pytest.mark.parametrize("ctor", ["opCholesky", "opInverse"])
def test_non_square_is_a_shape_mismatch_before_any_device_work(lo, ctor):
    """test/test_linop.jl:488 — CPU tensors: the check fires before the device is looked at."""
    for shape in ((3, 5), (5, 3)):
        with pytest.raises(lo.LinearOperatorException, match="shape mismatch"):
            getattr(lo, ctor)(torch.ones(shape, dtype=torch.float64))


@pytest.mark.parametrize("ctor", ["opCholesky", "opInverse"])
def test_complex_and_half_element_types_are_a_stated_limit(lo, ctor):
    for dt in (torch.complex128, torch.complex64):
        with pytest.raises(TypeError, match="real Float64 / Float32 only"):
            getattr(lo, ctor)(torch.eye(4, dtype=dt))
    with pytest.raises(TypeError):
        getattr(lo, ctor)(torch.eye(4, dtype=torch.float16))
    with pytest.raises(TypeError):
        getattr(lo, ctor)([[1.0, 0.0], [0.0, 1.0]])


@pytest.mark.parametrize("ctor", ["opCholesky", "opInverse"])
def test_a_host_matrix_is_refused_loudly(lo, ctor):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        getattr(lo, ctor)(torch.eye(4, dtype=torch.float64))
