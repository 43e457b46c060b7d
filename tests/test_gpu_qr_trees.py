"""-m gpu: opQR, opQR(pivot=True) and opPinv as LEAVES of operator trees. test_gpu_linalg_trees.py does this for the square
factorisations; a rectangular leaf owns ONE work area of 8 (mf + nf + 2·512·64) doubles that both of its modes rewrite, and
opPinv also shares W, T and perm with the pivoted operator it was built from, so a tree that applies the same leaf twice
(F.T * F, F + F, hcat(F, F), F * A * F), the transposed wrappers, Matrix(op), estimate_opnorm and a captured graph are where
sharing them could go wrong.

The generator is test_gpu_fuzz.Gen, subclassed as SolveGen is: the base class and its random stream are untouched, so the
seeds of the existing tests build the trees they always built. A leaf of shape (m, n) is the pseudo-inverse of an n x m matrix A:
  qr    opQR(A)               A = test_gpu_qr.simple_matrix (its transpose when n < m), singular values 1 .. 2, full rank
  qrp   opQR(A, pivot=True)   the same A
  pinv  opPinv(A)             A = test_gpu_qrp.deficient, rank max(1, min(m, n) // 2), singular values 1 .. 2
The dense model of a leaf is numpy's pinv (the deficient A with rcond = 1e-3, inside the gap between 0.5 and max(m, n) eps in both precisions), with
G = |pinv|."""
import numpy as np
import pytest
import torch

from test_gpu_fuzz import D, Gen, T, TM
from test_gpu_linalg_trees import check_tree, col_major
from test_gpu_qr_hard import build as rect_operator
from test_gpu_qrp import deficient, simple_matrix

pytestmark = pytest.mark.gpu
NB = 64
KINDS = ["qr", "qrp", "pinv"]
NP = {torch.float64: np.float64, torch.float32: np.float32}
DTYPES = [torch.float64, torch.float32]
DIDS = ["f64", "f32"]
BIG = (200, 129)


def rect_matrix(rng, kind, rows, cols):
    """the rows x cols matrix a leaf of `kind` pseudo-inverts (module docstring), Float64"""
    tall = rows >= cols
    mf, nf = (rows, cols) if tall else (cols, rows)
    A = deficient(rng, mf, nf, max(1, nf // 2)) if kind == "pinv" else simple_matrix(rng, mf, nf)
    return A if tall else np.ascontiguousarray(A.T)


def dense_pinv(kind, A):
    return np.linalg.pinv(A, rcond=1e-3) if kind == "pinv" else np.linalg.pinv(A)


class RectGen(Gen):
    """Gen whose leaves are, half of the time, one of the three rectangular solves (every shape allows one)"""

    def rect_leaf(self, kind, m, n):
        A = rect_matrix(self.rng, kind, n, m)
        X = dense_pinv(kind, A)
        op = rect_operator(self.lo, kind, TM(A, self.dev))
        if kind != "qr":
            assert op._rank == (max(1, min(m, n) // 2) if kind == "pinv" else min(m, n)), (kind, m, n, op._rank)
        return op, D(X, np.abs(X)), True, True, f"{kind}+[{m}x{n}]"

    def leaf(self, m, n):
        if self.rng.random() < 0.5:
            return self.rect_leaf(KINDS[self.rng.integers(len(KINDS))], m, n)
        return super().leaf(m, n)


# seeds 0 .. 11: each kind once as the pseudo-inverse of a tall and once of a wide matrix, at two and at three block columns
FORCED = [(kind, shape) for shape in ((65, 130), (130, 65), (129, 200), (200, 129)) for kind in KINDS]


@pytest.mark.parametrize("seed", range(40))
def test_random_operator_tree_with_rectangular_leaves_vs_dense(lo, dev, seed):
    """Seeds 0 .. 11 force a leaf F of shape (p, q) (FORCED) and combine it with a random tree t by one of F + t, t - F (t is
    p x q), F * t, t * F.T (t is q x q); seeds 12 .. 39 are free trees of the sizes of test_gpu_fuzz.py. check_tree and its 1e-10
    are test_gpu_linalg_trees.py's."""
    g = RectGen(lo, dev, 81000 + seed)
    rng = g.rng
    if seed < len(FORCED):
        kind, (p, q) = FORCED[seed]
        f, F, _, _, df = g.rect_leaf(kind, p, q)
        c = seed % 4
        t, Tt, tN, tT, dt = g.honouring_both(*((p, q) if c < 2 else (q, q)), depth=int(rng.integers(1, 3)))
        if c == 0:
            tree = (f + t, F + Tt, tN, tT, f"({df} + {dt})")
        elif c == 1:
            tree = (t - f, Tt - F, tN, tT, f"({dt} - {df})")
        elif c == 2:
            tree = (f * t, F @ Tt, True, tT, f"({df} * {dt})")
        else:
            tree = (t * f.T, Tt @ F.T, tN, True, f"({dt} * {df}.T)")
    else:
        hi = 13 if seed % 4 else 40
        m, n = int(rng.integers(1, hi)), int(rng.integers(1, hi))
        tree = g.tree(m, n, depth=int(rng.integers(1, 4)))
    check_tree(lo, dev, rng, *tree)


# ------------------------------------------------------------------------------------------------ the shared work area
def big_case(lo, dev, kind, dtype, seed):
    """(A, F, X, cond, rng): A 200 x 129 in the precision of dtype (pinv: rank 65), F its 129 x 200 leaf, X = pinv(A), cond = sigma_1 /
    sigma_r of the matrix the device holds"""
    npd = NP[dtype]
    rng = np.random.default_rng(seed)
    r = NB + 1 if kind == "pinv" else BIG[1]
    A = (deficient(rng, *BIG, r) if kind == "pinv" else simple_matrix(rng, *BIG)).astype(npd).astype(np.float64)
    F = rect_operator(lo, kind, col_major(A, dtype, dev))
    if kind != "qr":
        assert F._rank == r
    sv = np.linalg.svd(A, compute_uv=False)
    return A, F, dense_pinv(kind, A), float(sv[0] / sv[r - 1]), rng


@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("kind", KINDS)
def test_one_rectangular_leaf_applied_twice_in_a_tree(lo, dev, kind, dtype):
    """F = pinv(A), A 200 x 129 (pinv: rank 65): F.T * F, F * F.T, F + F, hcat(F, F), vcat(F, F) and F * A * F — which is
    F again, the second Penrose condition — on a vector and, column by column, on 3 columns (a product and a concatenation
    take vectors only; F + F and the leaf take the whole matrix). Tolerances as in
    test_gpu_linalg_trees.test_one_solve_applied_twice_in_a_tree: each solve contributes rel |its own result| once, rel =
    cond mf eps + 2 eps with cond = sigma_1 / sigma_r of A, and the error of an inner apply is carried through the outer ones by
    their 2-norms (first order). The dense product with A in F * A * F adds its own rounding, nf eps |A| |x| (a dot product of
    nf terms, gamma_nf to first order), carried by |pinv(A)|. The leaf on the whole matrix equals its columns bit for bit."""
    mf, nf = BIG
    npd = NP[dtype]
    eps = float(torch.finfo(dtype).eps)
    A, F, X, cond, rng = big_case(lo, dev, kind, dtype, 82000)
    assert tuple(F.shape) == (nf, mf) and cond <= 2.001
    nX, nA = np.linalg.norm(X, 2), np.linalg.norm(A, 2)
    rel = cond * mf * eps + 2 * eps
    Aop = lo.LinearOperatorFromMatrix(col_major(A, dtype, dev))
    V = rng.standard_normal((mf, 3)).astype(npd).astype(np.float64)           # operands with mf entries
    U = rng.standard_normal((nf, 3)).astype(npd).astype(np.float64)           # with nf entries
    V2 = rng.standard_normal((2 * mf, 3)).astype(npd).astype(np.float64)
    nrm = np.linalg.norm
    ops = (("F.T * F", F.T * F), ("F * F.T", F * F.T), ("F + F", F + F), ("hcat(F, F)", lo.hcat(F, F)), ("vcat(F, F)", lo.vcat(F, F)),
           ("F * A * F", F * Aop * F))

    def want(name, c):
        """(operand, expected result, tolerance) of column c"""
        v, u, v2 = V[:, c], U[:, c], V2[:, c]
        x = X @ v
        if name == "F.T * F":
            return v, X.T @ x, rel * (nX * nrm(x) + nrm(X.T @ x))
        if name == "F * F.T":
            xt = X.T @ u
            return u, X @ xt, rel * (nX * nrm(xt) + nrm(X @ xt))
        if name == "F + F":
            return v, 2 * x, 2 * rel * nrm(x) + eps * nrm(2 * x)
        if name == "hcat(F, F)":
            a, b = X @ v2[:mf], X @ v2[mf:]
            return v2, a + b, rel * (nrm(a) + nrm(b)) + eps * nrm(a + b)
        if name == "vcat(F, F)":
            return v, np.concatenate([x, x]), 2 * rel * nrm(x)
        return v, X @ (A @ x), rel * (nX * nA * nrm(x) + nrm(X @ (A @ x))) + nX * nf * eps * nA * nrm(x)

    for name, op in ops:
        v, ref, tol = want(name, 0)
        got = lo.apply(op, torch.from_numpy(v).to(dtype).to(dev)).cpu().numpy().astype(np.float64)
        print(f"{name} {kind} {dtype}: {nrm(got - ref) / tol:.3e} of the tolerance")
        assert nrm(got - ref) <= tol, (name, nrm(got - ref) / tol)
    for name, op in ops:
        Vin = np.stack([want(name, c)[0] for c in range(3)], axis=1)
        R = torch.full((3, op.shape[0]), float("nan"), dtype=dtype, device=dev).t()      # column-major
        Vd = col_major(Vin, dtype, dev)
        if name == "F + F":
            lo.mul(R, op, Vd)
        else:
            for c in range(3):
                lo.mul(R[:, c], op, Vd[:, c])
        got = R.cpu().numpy().astype(np.float64)
        for c in range(3):
            _, ref, tol = want(name, c)
            assert nrm(got[:, c] - ref) <= tol, (name, c, nrm(got[:, c] - ref) / tol)
    for w, M in ((F, V), (F.T, U)):                         # the leaf on the whole matrix: its columns, bit for bit
        Vd = col_major(M, dtype, dev)
        R = torch.full((3, w.shape[0]), float("nan"), dtype=dtype, device=dev).t()
        lo.mul(R, w, Vd)
        for c in range(3):
            assert torch.equal(R[:, c], lo.apply(w, Vd[:, c].clone())), c


@pytest.mark.parametrize("transposed", [False, True], ids=["tree", "tree.T"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_captured_tree_that_applies_one_rectangular_leaf_three_times_replays_bit_identically(lo, dev, kind, transposed):
    """capture_mul of F * A * F + F (and of its transpose) with (alpha, beta) = (2, -0.5): the replay equals the eager result bit for
    bit, a second replay after res and v were overwritten equals a fresh eager call on the new data, and the eager path is
    what it was."""
    dtype = torch.float64
    mf, nf = BIG
    A, F, _, _, rng = big_case(lo, dev, kind, dtype, 83000)
    op = F * lo.LinearOperatorFromMatrix(col_major(A, dtype, dev)) * F + F
    if transposed:
        op = op.T
    nout, nin = op.shape
    v1, v2 = (torch.from_numpy(rng.standard_normal(nin)).to(dev) for _ in range(2))
    r1, r2 = (torch.from_numpy(rng.standard_normal(nout)).to(dev) for _ in range(2))

    def eager(v, r0):
        res = r0.clone()
        lo.mul(res, op, v.clone(), 2.0, -0.5)
        return res

    want1, want2 = eager(v1, r1), eager(v2, r2)
    assert torch.isfinite(want1).all() and not torch.equal(want1, want2)
    v, res = v1.clone(), r1.clone()
    g = lo.capture_mul(res, op, v, 2.0, -0.5)
    res.copy_(r1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(res, want1)
    res.copy_(r2)
    v.copy_(v2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(res, want2)
    assert torch.equal(eager(v1, r1), want1)                # and the eager path is what it was


# ------------------------------------------------------------------------------------------------ estimate_opnorm
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("wide", [False, True], ids=["tall", "wide"])
@pytest.mark.parametrize("kind", ["qr", "pinv"])
def test_estimate_opnorm_of_a_rectangular_solve_is_one_over_the_smallest_singular_value(lo, dev, kind, wide, dtype):
    """opQR(A): 1 / sigma_min(A); opPinv(A) of rank 65: 1 / sigma_r(A). A is 200 x 129 or its transpose. The convention of
    test_gpu_opnorm.check: tol 1e-6 (Float32: 1e-3), converged is True, |value - ref| <= tol ref. One singular value is 0.25, the
    others 1 .. 2, so the top of the inverse's spectrum (4) is more than 5 % clear of the next value (<= 1). The reference is
    numpy's SVD of the matrix the device holds."""
    mf, nf = BIG
    npd = NP[dtype]
    r = nf if kind == "qr" else NB + 1
    rng = np.random.default_rng(84000)
    U = np.linalg.qr(rng.standard_normal((mf, r)))[0]
    V = np.linalg.qr(rng.standard_normal((nf, r)))[0]
    s = np.linspace(1.0, 2.0, r)
    s[r // 2] = 0.25
    A = ((U * s) @ V.T).astype(npd).astype(np.float64)
    if wide:
        A = np.ascontiguousarray(A.T)
    sv = np.linalg.svd(A, compute_uv=False)
    ref = 1.0 / sv[r - 1]
    assert 1.0 / sv[r - 2] <= 0.95 * ref
    assert r == nf or sv[r] <= 0.05 * max(mf, nf) * float(np.finfo(npd).eps) * sv[0]     # far below the rank threshold
    op = rect_operator(lo, kind, col_major(A, dtype, dev))
    if kind == "pinv":
        assert op._rank == r
    tol = 1e-6 if dtype == torch.float64 else 1e-3
    value, converged = lo.estimate_opnorm(op, tol=tol)
    print(f"estimate_opnorm({kind}) {'wide' if wide else 'tall'} {dtype}: {value!r} (reference {ref!r}, converged {converged})")
    assert converged is True and isinstance(value, float)
    assert abs(value - ref) <= tol * ref
