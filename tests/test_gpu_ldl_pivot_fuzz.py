"""-m gpu: randomised differential test of opLDL(M, pivot=True) (csrc/linalg.hip: mxlo_sytrf, mxlo_ldlp_mul, mxlo_ldlp_mul_block) at
the cases of tests/ldl_pivot_hard_cases.case: the three Gaussian families of ldl_pivot_cases.py and the four exact families at
random sizes (with n = 128, 192, 256 forced), both precisions, four storages of M, vector and block operands in their own
leading dimensions and element offsets behind guard zones, wrappers, scalars and the res-is-v alias.
tests/test_ldl_pivot_hard_host.py (CPU) shows that LAPACK in the same precision meets the bound at every seed with a factor of
two to spare.

Per seed, the seven checks of test_gpu_linalg_fuzz.test_random_case: (1) the constructor leaves the matrix, its padding and
guards bit-unchanged; (2) the plain apply of the drawn wrapper to a NaN-filled res is finite and eta <= 3 n eps(T) for every
column — the DERIVED bound of ldl_pivot_cases.py, computed on the host in Float64 from the matrix the device saw; (3) the apply
with the drawn (alpha, beta) equals alpha x + beta res0 to 4 eps(T) (|alpha x| + |beta res0|), derived in test_gpu_linalg_fuzz.py;
(4) every column of a block apply has the bits of its vector apply; (5) nothing outside res is written; (6) a second run gives
the same bits; (7) where drawn, mul!(x, op, x) has the bits of the separate-buffer call. And of the factor: perm is a
permutation, e[k] != 0 => e[k + 1] == 0, every 2 x 2 block has a negative determinant, the inertia is the sign count of the
eigenvalues (wherever no eigenvalue lies within 1000 backward errors 3 n eps(T) |M| of zero: a backward-stable factorisation has
the inertia of a matrix that close, which a Float32 saddle0 with a square B does not pin down; the host test counts how many
seeds of each family qualify), and for the exact families perm, d, e, L and the inertia are the rational model's bit for bit.
MXLO_LDLPFUZZ_SEEDS extends the list of seeds."""
import numpy as np
import pytest
import torch

import ldl_pivot_hard_cases as hc
import linalg_fuzz_cases as fz
import test_gpu_ldl_pivot as tp
import test_gpu_linalg_fuzz as lf

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", hc.seeds())
def test_random_case(lo, dev, seed):
    c = hc.case(seed)
    n = c.n
    dtype = lf.TORCH[c.npd]
    tag = f"ldlpfuzz seed={seed} {c.family} n={n} {c.npd.__name__} {c.storage}{'-row' if c.rowmajor else ''} k={c.k} {c.wrapper}"
    # ---- 1. build
    mflat, Md = lf.upload(fz.matrix_storage(c), dev)
    mbefore = mflat.clone()
    assert tuple(Md.shape) == (n, n) and Md.data_ptr() == mflat.data_ptr() + c.off * mflat.element_size()
    op = lo.opLDL(Md, pivot=True)
    assert lf.same_bits(mflat, mbefore), "the constructor wrote to the matrix, its padding or its guards"
    assert tuple(op.shape) == (n, n) and op.eltype is dtype and op.symmetric and op.hermitian and op._refine == 0
    w = {"op": lambda o: o, "transpose": lo.transpose, "adjoint": lo.adjoint}[c.wrapper](op)
    assert tuple(lo.size(w)) == (n, n)
    # ---- the factor
    L, d, e, perm = tp.read_factor(op, n)
    assert sorted(perm.tolist()) == list(range(n)), tag
    two = np.nonzero(e)[0]
    assert e[n - 1] == 0.0 and not e[two + 1].any(), tag
    assert (d[two] * d[two + 1] - e[two] * e[two] < 0).all(), tag
    if c.inertia_checked:                                       # no eigenvalue within 1000 backward errors of zero
        assert lo.ldl_inertia(op) == (int((c.eig > 0).sum()), int((c.eig < 0).sum()), 0), tag
    if c.exact:
        mperm, mL, md, me, inertia = hc.exact_factor(c.family, c.args)
        assert lo.ldl_inertia(op) == inertia == (int((c.eig > 0).sum()), int((c.eig < 0).sum()), 0), tag
        assert np.array_equal(perm, mperm) and np.array_equal(d, md) and np.array_equal(e, me), tag
        assert np.array_equal(np.tril(L, -1), np.tril(mL, -1)), tag
    # ---- 2. accuracy of the plain apply on a NaN-filled res
    vstore = fz.operand_storage(c.V.astype(c.npd), c.ldv, c.offv, np.nan)
    vflat, V = lf.upload(vstore, dev, c.vector)
    vbefore = vflat.clone()
    nan_store = fz.operand_storage(np.full((n, c.k), np.nan, dtype=c.npd), c.ldr, c.offr, fz.RES_SENTINEL)
    rflat, R = lf.upload(nan_store, dev, c.vector)
    lo.mul(R, w, V)
    X = lf.host2d(R)
    assert np.isfinite(X).all(), tag
    assert lf.untouched_outside(rflat, nan_store), tag
    ratio = hc.worst_eta(c, X)
    print(f"{tag} eta: {ratio:.3e} of the bound")
    assert ratio <= 1.0, (tag, ratio)                           # 3 n eps(T): derived (ldl_pivot_cases.py)
    # ---- 3. the drawn scalars against alpha x + beta res0
    a, b = c.scalars if c.scalars is not None else (1.0, 0.0)
    rstore = fz.operand_storage(c.res0.astype(c.npd), c.ldr, c.offr, fz.RES_SENTINEL)
    rflat, R = lf.upload(rstore, dev, c.vector)
    lf.apply(lo, R, w, V, c.scalars)
    got = lf.host2d(R)
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
            lf.apply(lo, r, w, v, c.scalars)
            assert lf.same_bits(R[:, j].contiguous(), r), (tag, "column", j)
    # ---- 5. nothing else is written
    assert lf.untouched_outside(rflat, rstore), tag
    assert lf.same_bits(vflat, vbefore), tag
    assert lf.same_bits(mflat, mbefore), tag
    # ---- 6. reproducible
    r2flat, R2 = lf.upload(rstore, dev, c.vector)
    lf.apply(lo, R2, w, V, c.scalars)
    assert lf.same_bits(r2flat, rflat), tag
    # ---- 7. res is v
    if c.alias:
        sflat, S = lf.operand(c, c.V, c.ldr, c.offr, fz.RES_SENTINEL, dev)  # separate buffers, res holding a copy of V
        lf.apply(lo, S, w, V, c.scalars)
        xflat, Xv = lf.upload(vstore, dev, c.vector)
        lf.apply(lo, Xv, w, Xv, c.scalars)
        assert lf.same_bits(Xv.contiguous(), S.contiguous()), tag
        assert lf.untouched_outside(xflat, vstore), tag
