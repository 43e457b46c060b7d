"""CPU: the host half of opQR (the rectangular dense `M \\ v` of src/linalg.jl:27-32) — the public name, the C-ABI
declarations it rests on, the refusals that happen before any device work and their order, and the launch count the
apply promises. No device call anywhere in this file."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mxlo_geqrf", "mxlo_qr_mul")


def test_public_name_header_declarations_and_exports(lo):
    assert callable(lo.opQR)
    syms = lo._lib.header_symbols()
    L = lo._lib.lib()
    for name in ENTRY_POINTS:
        assert name in syms and name in lo._lib._PROTOS, name
        assert hasattr(L, name), name                       # exported by the built library


def test_the_source_that_holds_the_entry_points_is_built(lo):
    csrc = os.path.join(ROOT, "linearoperators.jl_amd", "csrc")
    holders = set()
    for fn in sorted(os.listdir(csrc)):
        if fn.endswith(".hip"):
            with open(os.path.join(csrc, fn)) as f:
                src = f.read()
            if all(f"int32_t {name}(" in src for name in ENTRY_POINTS):
                holders.add(fn)
    assert holders
    with open(os.path.join(csrc, "Makefile")) as f:
        mk = f.read()
    assert all(fn in mk for fn in holders)


def test_refusals_fire_in_the_stated_order_without_a_device(lo):
    with pytest.raises(TypeError):                                        # not a 2-D tensor
        lo.opQR([[1.0, 0.0], [0.0, 1.0]])
    with pytest.raises(TypeError):
        lo.opQR(torch.ones(4, dtype=torch.float64))
    for shape in ((0, 3), (3, 0), (0, 0)):                                # a zero dimension, before the element type
        with pytest.raises(lo.LinearOperatorException):
            lo.opQR(torch.ones(shape, dtype=torch.complex128))
    for dt in (torch.complex128, torch.complex64, torch.float16, torch.bfloat16):   # the element type, before the device
        with pytest.raises(TypeError, match="real Float64 / Float32 only"):
            lo.opQR(torch.ones((5, 3), dtype=dt))
    for dt in (torch.float64, torch.float32):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            lo.opQR(torch.eye(4, dtype=dt))


def test_rectangular_is_not_a_shape_mismatch(lo):
    for shape in ((3, 5), (5, 3)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            lo.opQR(torch.ones(shape, dtype=torch.float64))


def test_launch_count_is_within_the_promise_and_knows_no_row_count(lo):
    import inspect
    assert list(inspect.signature(lo.linalg.qr_launches).parameters) == ["nf"]
    for nf in (1, 63, 64, 65, 129, 4097):
        nblk = -(-nf // 64)
        got = lo.linalg.qr_launches(nf)
        assert isinstance(got, int) and 1 <= got <= 3 * nblk + 2, (nf, got)
