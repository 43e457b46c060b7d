"""-m gpu: randomised differential test of the factorisation operators (csrc/linalg.hip, linearoperators.jl_amd/linalg.py) —
opCholesky, opLDL, opLU, triangular opInverse, opQR with and without pivot=True, opPinv — at the cases of
tests/linalg_fuzz_cases.py: random shapes (with every multiple of the block width 64 up to 256 and the forced shapes the pinned
files leave out), element types, storage orders, padded leading dimensions, base pointers off the 16-byte phase, vector and
block operands in their own leading dimensions and offsets, wrappers, scalars, `refine` and `rtol`.
tests/test_linalg_fuzz_host.py (CPU) shows that LAPACK in the same precision meets every bound used here with a factor of two
to spare at every seed, and the drawn rank with a factor of 20 on both sides of the threshold.

Per seed: (1) the constructor leaves the matrix, its padding and guards bit-unchanged and reports the expected rank, triangle,
orientation and refine; (2) the plain apply of the drawn wrapper to a NaN-filled res is finite and inside the family's DERIVED
bound — n eps(T), n eps(T) rho, mf eps(T): the docstrings of the pinned files — for every column, computed on the host in
Float64 from the matrix the device saw; (3) the apply with the drawn (alpha, beta) equals alpha x + beta res0 elementwise with x
the device's own result of (2), to 4 eps(T) (|alpha x| + |beta res0|): the kernels form alpha x + beta res in Float64 and round
once to T, and (2) is that same x rounded once to T, so the two differ by at most u |alpha x| + u |res| <= eps (|alpha x| +
|beta res0|) with u = eps / 2; the factor 4 covers the host's own three roundings. Derived, not measured. (4) every column of a
block apply has the bits of its vector apply; (5) nothing outside res is written: the padding of res, both guard zones, V and
the matrix keep their bits; (6) a second run gives the same bits; (7) where drawn, mul!(x, op, x) has the bits of the
separate-buffer call. MXLO_LINFUZZ_SEEDS extends the list of seeds."""
import numpy as np
import pytest
import torch

import linalg_fuzz_cases as fz

pytestmark = pytest.mark.gpu
TORCH = {np.float64: torch.float64, np.float32: torch.float32}


def upload(storage, dev, vector=False):
    """(flat device buffer, view of the window) of a (buffer, shape, strides, offset) from linalg_fuzz_cases"""
    buf, shape, strides, offset = storage
    flat = torch.from_numpy(buf).to(dev)
    if vector:
        return flat, flat.as_strided((shape[0],), (1,), offset)
    return flat, flat.as_strided(shape, strides, offset)


def bits(t):
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def host2d(view):
    return view.detach().cpu().numpy().astype(np.float64).reshape(view.shape[0], -1)


def construct(lo, c, Md):
    if c.family == "chol":
        return lo.opCholesky(Md, refine=c.refine)
    if c.family == "ldl":
        return lo.opLDL(Md, refine=c.refine)
    if c.family == "lu":
        return lo.opLU(Md, refine=c.refine)
    if c.family in ("lower", "upper"):
        return lo.opInverse(Md)
    if c.family == "qr":
        return lo.opQR(Md)
    if c.family == "qrp":
        return lo.opQR(Md, pivot=True, rtol=c.rtol)
    return lo.opPinv(Md, rtol=c.rtol)


def operand(c, X, ld, off, sentinel, dev):
    return upload(fz.operand_storage(np.ascontiguousarray(X).astype(c.npd), ld, off, sentinel), dev, c.vector)


def apply(lo, res, w, V, scalars):
    if scalars is None:
        lo.mul(res, w, V)
    else:
        lo.mul(res, w, V, *scalars)


def untouched_outside(flat, storage):
    """the elements of the flat device buffer outside the window still hold the bits they were uploaded with"""
    buf, shape, strides, offset = storage
    return np.array_equal(fz.outside(flat.cpu().numpy(), shape, strides, offset), fz.outside(buf, shape, strides, offset))


@pytest.mark.parametrize("seed", fz.seeds())
def test_random_case(lo, dev, seed):
    c = fz.case(seed)
    dtype = TORCH[c.npd]
    tag = f"linfuzz seed={seed} {c.family} {c.shape} {c.npd.__name__} {c.storage}{'-row' if c.rowmajor else ''} k={c.k} {c.wrapper}"
    # ---- 1. build
    mflat, Md = upload(fz.matrix_storage(c), dev)
    mbefore = mflat.clone()
    assert tuple(Md.shape) == c.A.shape and Md.data_ptr() == mflat.data_ptr() + c.off * mflat.element_size()
    op = construct(lo, c, Md)
    assert same_bits(mflat, mbefore), "the constructor wrote to the matrix, its padding or its guards"
    assert tuple(op.shape) == (c.A.shape[1], c.A.shape[0]) and op.eltype is dtype
    if c.family in fz.REFINABLE:
        assert op._refine == c.refine
    if c.family in ("lower", "upper"):
        assert op._triangle == c.family
    if not c.square:
        assert op._tall == (c.A.shape[0] >= c.A.shape[1])
    if c.family in ("qrp", "pinv"):
        assert op._rank == c.rank, (op._rank, c.rank)
        assert op._rtol == c.rtol_value
    w = {"op": lambda o: o, "transpose": lo.transpose, "adjoint": lo.adjoint}[c.wrapper](op)
    assert tuple(lo.size(w)) == (c.rows_out, c.rows_in)
    # ---- 2. accuracy of the plain apply on a NaN-filled res
    vstore = fz.operand_storage(c.V.astype(c.npd), c.ldv, c.offv, np.nan)
    vflat, V = upload(vstore, dev, c.vector)
    vbefore = vflat.clone()
    nan_store = fz.operand_storage(np.full((c.rows_out, c.k), np.nan, dtype=c.npd), c.ldr, c.offr, fz.RES_SENTINEL)
    rflat, R = upload(nan_store, dev, c.vector)
    lo.mul(R, w, V)
    X = host2d(R)
    assert np.isfinite(X).all(), tag
    assert untouched_outside(rflat, nan_store), tag
    for name, ratio in fz.ratios(c, X).items():
        print(f"{tag} {name}: {ratio:.3e} of the bound")
        assert ratio <= 1.0, (tag, name, ratio)                 # the derived bounds of the pinned files (module docstring)
    if c.family == "qrp" and c.lsq:                             # the basic solution: exactly zero outside the r pivots
        free = op._perm.cpu().numpy()[c.rank:]
        assert (X[free] == 0.0).all() and sorted(op._perm.cpu().tolist()) == list(range(c.nf)), tag
    # ---- 3. the drawn scalars against alpha x + beta res0
    a, b = c.scalars if c.scalars is not None else (1.0, 0.0)
    rstore = fz.operand_storage(c.res0.astype(c.npd), c.ldr, c.offr, fz.RES_SENTINEL)
    rflat, R = upload(rstore, dev, c.vector)
    apply(lo, R, w, V, c.scalars)
    got = host2d(R)
    if b == 0:
        assert np.isfinite(got).all(), tag                      # beta == 0: res is not read, its NaN included
        want, scale = a * X, np.abs(a * X)
    else:
        want, scale = a * X + b * c.res0, np.abs(a * X) + np.abs(b * c.res0)
    excess = np.abs(got - want) - 4 * c.eps * scale
    assert (excess <= 0).all(), (tag, c.scalars, float(np.max(np.abs(got - want) / np.where(scale > 0, scale, 1.0)) / c.eps))
    # ---- 4. every column of a block apply is its vector apply, bit for bit
    if not c.vector:
        for j in range(c.k):
            r = torch.from_numpy(c.res0[:, j].astype(c.npd)).to(dev)
            v = torch.from_numpy(c.V[:, j].astype(c.npd)).to(dev)
            apply(lo, r, w, v, c.scalars)
            assert same_bits(R[:, j].contiguous(), r), (tag, "column", j)
    # ---- 5. nothing else is written
    assert untouched_outside(rflat, rstore), tag
    assert same_bits(vflat, vbefore), tag
    assert same_bits(mflat, mbefore), tag
    # ---- 6. reproducible
    r2flat, R2 = upload(rstore, dev, c.vector)
    apply(lo, R2, w, V, c.scalars)
    assert same_bits(r2flat, rflat), tag
    # ---- 7. res is v
    if c.alias:
        sflat, S = operand(c, c.V, c.ldr, c.offr, fz.RES_SENTINEL, dev)     # separate buffers, res holding a copy of V
        apply(lo, S, w, V, c.scalars)
        xflat, Xv = upload(vstore, dev, c.vector)
        apply(lo, Xv, w, Xv, c.scalars)
        assert same_bits(Xv.contiguous(), S.contiguous()), tag
        assert untouched_outside(xflat, vstore), tag
