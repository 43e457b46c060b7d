"""-m gpu: opCholesky, opLDL, opLU and triangular opInverse as LEAVES of operator trees. test_gpu_fuzz.py grows its trees
from every other leaf of the hot path; each of these four owns ONE f64 work vector that every apply rewrites, so a tree that
applies the same solve twice (F * F, F + F, hcat(F, F)), the transposed wrappers, Matrix(op), estimate_opnorm and a captured
graph are where sharing it could go wrong.

The generator is test_gpu_fuzz.Gen, subclassed: the base class and its random stream are untouched, so the seeds of
test_random_operator_tree_vs_dense build the trees they always built. Matrices are well conditioned by construction
(condition number <= 4): SPD H = Q diag(1 .. 3) Q'; the quasi-definite K flips the sign of H where both indices are
2 mod 3 (a symmetric permutation of [A B'; B -C] with the spectra of A, C in [1, 3] and |B|_2 <= 1, so |K|_2 <= 4 and its
singular values are >= 1); U S V' with singular values 1 .. 2; the Cholesky factor of H and its transpose. The dense model of
a solve is numpy's inverse, with G = |inv(A)|."""
import numpy as np
import pytest
import torch

from test_gpu_fuzz import D, Gen, T, TM

pytestmark = pytest.mark.gpu
NB = 64
KINDS = ["chol", "ldl", "lu", "lower", "upper"]             # opInverse counts once, with both triangles
NP = {torch.float64: np.float64, torch.float32: np.float32}


def solve_matrix(rng, kind, n):
    """the matrix a solve leaf of `kind` inverts, Float64, condition number <= 4 (module docstring)"""
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    H = (Q * np.linspace(1.0, 3.0, n)) @ Q.T
    H = (H + H.T) / 2
    if kind == "chol":
        return H
    if kind == "ldl":
        s = np.where(np.arange(n) % 3 == 2, -1.0, 1.0)
        return np.where((s[:, None] < 0) & (s[None, :] < 0), -H, H)
    if kind == "lu":
        V = np.linalg.qr(rng.standard_normal((n, n)))[0]
        return (Q * np.linspace(1.0, 2.0, n)) @ V.T
    L = np.linalg.cholesky(H)
    return L if kind == "lower" else np.ascontiguousarray(L.T)


def solve_operator(lo, kind, Ad):
    return {"chol": lo.opCholesky, "ldl": lo.opLDL, "lu": lo.opLU, "lower": lo.opInverse, "upper": lo.opInverse}[kind](Ad)


class SolveGen(Gen):
    """Gen whose square leaves are, half of the time, one of the four solves"""

    def solve_leaf(self, kind, n):
        A = solve_matrix(self.rng, kind, n)
        X = np.linalg.inv(A)
        return solve_operator(self.lo, kind, TM(A, self.dev)), D(X, np.abs(X)), True, True, f"{kind}^-1[{n}x{n}]"

    def leaf(self, m, n):
        if m == n and self.rng.random() < 0.5:
            return self.solve_leaf(KINDS[self.rng.integers(len(KINDS))], n)
        return super().leaf(m, n)


def check_tree(lo, dev, rng, op, DM, honours, honours_t, desc):
    """the four checks and the tolerance of test_gpu_fuzz.test_random_operator_tree_vs_dense"""
    M = DM.M
    m, n = M.shape
    assert op.shape == (m, n)
    v, w, r0 = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)
    scale = max(np.linalg.norm(DM.G, 2), 1e-300)

    def close(got, want, vec, extra=0.0):
        return np.linalg.norm(got - want) <= 1e-10 * (scale * np.linalg.norm(vec) + extra)

    assert close((op * T(v, dev)).cpu().numpy(), M @ v, v), desc
    assert close((op.T * T(w, dev)).cpu().numpy(), M.T @ w, w), desc
    assert close((op.H * T(w, dev)).cpu().numpy(), M.T @ w, w), desc
    res = T(r0.copy(), dev)
    lo.mul(res, op, T(v, dev), 3.0, -4.0)
    if honours:
        assert close(res.cpu().numpy(), 3.0 * (M @ v) - 4.0 * r0, 3 * v, 4 * np.linalg.norm(r0)), desc
    if honours_t:
        rt0 = rng.standard_normal(n)
        rt = T(rt0.copy(), dev)
        lo.mul(rt, op.T, T(w, dev), 3.0, -4.0)
        assert close(rt.cpu().numpy(), 3.0 * (M.T @ w) - 4.0 * rt0, 3 * w, 4 * np.linalg.norm(rt0)), desc
    assert np.linalg.norm(lo.Matrix(op).cpu().numpy() - M) <= 1e-10 * scale * max(m, n), desc


FORCED = [(kind, n) for n in (NB + 1, 2 * NB + 1) for kind in KINDS]       # seeds 0 .. 9: the multi-launch chain inside a tree


@pytest.mark.parametrize("seed", range(60))
def test_random_operator_tree_with_solve_leaves_vs_dense(lo, dev, seed):
    """Seeds 0 .. 9 force each kind once at n = NB + 1 and once at 2 NB + 1 (two and three block columns): the forced leaf F
    is combined with a random n x n tree t by one of F + t, t - F, F * t, t * F.T; seeds 10 .. 59 are free trees of the
    sizes of the existing test whose square leaves are solves half of the time, and seeds 10 .. 14 put one kind each at the
    root of a product so that every kind also appears at a small size."""
    g = SolveGen(lo, dev, 77000 + seed)
    rng = g.rng
    if seed < len(FORCED):
        kind, n = FORCED[seed]
        f, F, _, _, df = g.solve_leaf(kind, n)
        t, Tt, tN, tT, dt = g.honouring_both(n, n, depth=int(rng.integers(1, 3)))
        c = seed % 4
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
        if seed < len(FORCED) + len(KINDS):
            f, F, _, _, df = g.solve_leaf(KINDS[seed - len(FORCED)], m)
            tree = (f * tree[0], F @ tree[1], True, tree[3], f"({df} * {tree[4]})")
    check_tree(lo, dev, rng, *tree)


# ------------------------------------------------------------------------------------------------ the shared work vector
def per_solve_rel(kind, A, n, eps):
    """the relative tolerance of ONE solve in the alpha / beta tests of test_gpu_linalg.py, test_gpu_ldl.py and
    test_gpu_lu.py: cond(A) n eps (times rho = | |L||D||L'| |_2 / |K|_2 for opLDL) + 2 eps"""
    rel = np.linalg.cond(A) * n * eps
    if kind == "ldl":
        from test_gpu_ldl import facts
        rel *= facts(A)[5]
    return rel + 2 * eps


def col_major(A, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(A).T)).to(dtype).to(dev).t()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_one_solve_applied_twice_in_a_tree(lo, dev, kind, dtype):
    """F * F, F + F, F * F.T and hcat(F, F) on a vector and on an n x 3 matrix against numpy. Each solve contributes its
    per-solve tolerance once: rel |its own result|, and the error of an inner solve is carried through the outer one by
    |inv(A)|_2 (first order). The package defines mul! on matrices for leaves, sums and scalar multiples; a product and an
    hcat refuse a matrix operand (asserted here), so these go over the n x 3 matrix column by column, res and v being the
    strided columns of two column-major buffers. F + F and the leaf F itself take the whole matrix, and F must give the
    same bits as its columns."""
    n, npd = 2 * NB + 1, NP[dtype]
    eps = float(torch.finfo(dtype).eps)
    rng = np.random.default_rng(78000)
    A = solve_matrix(rng, kind, n).astype(npd).astype(np.float64)
    F = solve_operator(lo, kind, col_major(A, dtype, dev))
    X = np.linalg.inv(A)
    nX = np.linalg.norm(X, 2)
    rel = per_solve_rel(kind, A, n, eps)
    V = rng.standard_normal((n, 3)).astype(npd).astype(np.float64)
    V2 = rng.standard_normal((2 * n, 3)).astype(npd).astype(np.float64)
    nrm = np.linalg.norm

    def cases(v, v2):
        x, xt = X @ v, X.T @ v
        return (("F * F", F * F, v, X @ x, rel * (nX * nrm(x) + nrm(X @ x))),
                ("F + F", F + F, v, 2 * x, 2 * rel * nrm(x) + eps * nrm(2 * x)),
                ("F * F.T", F * F.T, v, X @ xt, rel * (nX * nrm(xt) + nrm(X @ xt))),
                ("hcat(F, F)", lo.hcat(F, F), v2, X @ v2[:n] + X @ v2[n:], rel * (nrm(X @ v2[:n]) + nrm(X @ v2[n:])) + eps * nrm(X @ v2[:n] + X @ v2[n:])))

    for name, op, v, want, tol in cases(V[:, 0], V2[:, 0]):
        got = lo.apply(op, torch.from_numpy(v).to(dtype).to(dev)).cpu().numpy().astype(np.float64)
        assert nrm(got - want) <= tol, (name, nrm(got - want) / tol)
    for j, (name, op, _, _, _) in enumerate(cases(V[:, 0], V2[:, 0])):
        Vin = V2 if name.startswith("hcat") else V
        R = torch.full((n, 3), float("nan"), dtype=dtype, device=dev).t().contiguous().t()      # column-major
        Vd = col_major(Vin, dtype, dev)
        if name == "F + F":
            lo.mul(R, op, Vd)
        else:
            with pytest.raises(lo.LinearOperatorException, match="vectors only"):
                lo.mul(R, op, Vd)
            assert torch.isnan(R).all()                     # refused before anything was launched
            for c in range(3):
                lo.mul(R[:, c], op, Vd[:, c])
        got = R.cpu().numpy().astype(np.float64)
        for c in range(3):
            _, _, _, want, tol = cases(V[:, c], V2[:, c])[j]
            assert nrm(got[:, c] - want) <= tol, (name, c, nrm(got[:, c] - want) / tol)
    Vd = col_major(V, dtype, dev)                           # the leaf on the whole matrix: its columns, bit for bit
    R = torch.full((n, 3), float("nan"), dtype=dtype, device=dev).t().contiguous().t()
    lo.mul(R, F, Vd)
    for c in range(3):
        assert torch.equal(R[:, c], lo.apply(F, Vd[:, c].clone())), c


@pytest.mark.parametrize("kind", KINDS)
def test_a_captured_tree_that_applies_one_solve_three_times_replays_bit_identically(lo, dev, kind):
    """capture_mul of F * F + F: the replay equals the eager result bit for bit, and a second replay after res and v were
    overwritten equals a fresh eager call on the new data."""
    n, dtype = 2 * NB + 1, torch.float64
    rng = np.random.default_rng(79000)
    F = solve_operator(lo, kind, col_major(solve_matrix(rng, kind, n), dtype, dev))
    op = F * F + F
    v1, v2, r1, r2 = (torch.from_numpy(rng.standard_normal(n)).to(dev) for _ in range(4))

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
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["lu", "chol"])
def test_estimate_opnorm_of_a_solve_is_one_over_sigma_min(lo, dev, kind, dtype):
    """The convention of test_gpu_opnorm.check: tol 1e-6 (Float32: 1e-3), converged is True, |value - ref| <= tol ref; the
    chosen spectrum keeps the top of the inverse's (1 / 0.25 = 4) more than 5 % away from the next value (<= 1), as that
    file requires of the spectra it picks. The reference is 1 / sigma_min of the matrix the device holds, from numpy."""
    n, npd = 2 * NB + 1, NP[dtype]
    rng = np.random.default_rng(80000)
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    V = Q if kind == "chol" else np.linalg.qr(rng.standard_normal((n, n)))[0]
    s = np.linspace(1.0, 2.0, n)
    s[n // 2] = 0.25
    A = (Q * s) @ V.T
    if kind == "chol":
        A = (A + A.T) / 2
    A = A.astype(npd).astype(np.float64)
    sv = np.linalg.svd(A, compute_uv=False)
    ref = 1.0 / sv[-1]
    assert 1.0 / sv[-2] <= 0.95 * ref
    op = solve_operator(lo, kind, col_major(A, dtype, dev))
    tol = 1e-6 if dtype == torch.float64 else 1e-3
    value, converged = lo.estimate_opnorm(op, tol=tol)
    print(f"estimate_opnorm({kind}^-1) {dtype}: {value!r} (1 / sigma_min {ref!r}, converged {converged})")
    assert converged is True and isinstance(value, float)
    assert abs(value - ref) <= tol * ref
