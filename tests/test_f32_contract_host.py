"""CPU: the Float32 contract test of test_gpu_f32_contract.py has teeth before it sees a device. At every family and shape of
f32_contract_cases.py
  - the set F_i never holds more than two adjacent floats (per component);
  - a NumPy model that accumulates in Float64 and rounds once is inside the expected set for every (alpha, beta);
  - a model that accumulates in Float32 — sequentially, and NumPy's own `W32 @ x32` — is outside it on at least one element;
  - a Float64-accumulated model that drops one term, or doubles one, is outside it.
The shapes in f32_contract_cases.EDGE_ONLY are "edge only" (they stay in the GPU test for their raggedness): inside is asserted,
the Float32-accumulation teeth are not, and for those also in TAMPER_ONLY the dropped and the doubled term still are. Each case prints the median and the worst cancellation ratio S_i / |y_i| of its inputs (pytest -s)."""
import numpy as np
import pytest

import f32_contract_cases as cc
import forms_cases as fc

F32, C64 = cc.F32, cc.C64


def wide(a):
    return a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)


def acc64(W, x):
    """accumulate in Float64 (any order), round once"""
    return (wide(W) @ wide(x)).astype(W.dtype)


def acc32_seq(W, x):
    """accumulate sequentially in the element type"""
    if W.shape[0] == 1:
        return np.cumsum(W[0] * x, dtype=W.dtype)[-1:].copy()
    acc = np.zeros(W.shape[0], W.dtype)
    for j in range(W.shape[1]):
        acc = acc + W[:, j] * x[j]
    return acc


def acc32_blas(W, x):
    return np.ascontiguousarray(W) @ x


def tampered(W, x, factor):
    """Float64 accumulation with the term of one reduced index dropped (factor 0) or doubled (factor 2)"""
    j = W.shape[1] // 3
    xx = wide(x)
    xx[j] *= factor
    return (wide(W) @ xx).astype(W.dtype), j


def teeth_of(case):
    """True: all teeth; "tamper": the lost / doubled term only; False: none (f32_contract_cases.EDGE_ONLY)"""
    if case not in cc.EDGE_ONLY:
        return True
    print(f"{case}: edge only")
    return "tamper" if case in cc.TAMPER_ONLY else False


def check(name, W, x, s, out_of, cands_of, teeth=True, touched=None, every=True):
    """out_of(f, ab): the output for rounded sums f; cands_of(ab): the candidate outputs"""
    W = np.atleast_2d(W)
    assert s.sizes.max() <= 2, (name, "a set F_i holds more than two floats", int(np.argmax(s.sizes)))
    print(f"{name}: cancellation ratio S_i / |y_i| median {s.ratio:.0f}, worst {s.ratio_max:.0f}, terms {s.terms}, largest |F_i| {int(s.sizes.max())}")
    f64 = acc64(W, x)
    for ab in cc.SCALARS:
        ok = cc.member(out_of(f64, ab), cands_of(ab))
        assert ok.all(), (name, ab, "the Float64-accumulated model leaves the set at", int(np.flatnonzero(~ok)[0]))
    if not teeth:
        return
    for ab in cc.SCALARS[:2]:
        cands = cands_of(ab)
        for label, f in (("sequential Float32", acc32_seq(W, x)), ("W32 @ x32", acc32_blas(W, x))) if teeth is True else ():
            assert not cc.member(out_of(f, ab), cands).all(), (name, ab, label, "accumulation stays inside the set")
        for factor in (0.0, 2.0):
            f, j = tampered(W, x, factor)
            ok = cc.member(out_of(f, ab), cands)
            hit = np.flatnonzero(np.abs(W[:, j]) > 0) if touched is None else touched(j)
            assert hit.size and not (ok[hit].any() if every else ok.all()), (name, ab, f"term {j} x {factor}", "stays inside the set")


@pytest.mark.parametrize("t,n", [(t, n) for t in ("f32", "c64") for n in cc.DOT_SIZES[t]])
def test_dot(t, n):
    a, b, s = cc.dot_case(t, n)
    W = np.conj(a)[None, :] if t == "c64" else a[None, :]
    check(f"dot {t} {n}", W, b, s, lambda f, ab: f, lambda ab: s.F, teeth=teeth_of(("dot", t, n)))


@pytest.mark.parametrize("t,n", [(t, n) for t in ("f32", "c64") for n in cc.HOUSE_SIZES[t]] + [("f32", cc.kept_n(256))])
def test_householder(t, n):
    h, v, r0, s = cc.house_case(t, n)
    cplx = t == "c64"
    W = np.conj(h)[None, :] if cplx else h[None, :]
    out_of = lambda f, ab: cc.epi_of(cplx)(cc.house_model(h, v, f[0], cplx), r0, ab)
    check(f"householder {t} {n}", W, v, s, out_of, lambda ab: cc.house_candidates(t, n, ab), teeth=teeth_of(("house", t, n)),
          every=False)


def test_householder_has_teeth_somewhere():
    for t in ("f32", "c64"):
        assert any(("house", t, n) not in cc.EDGE_ONLY for n in cc.HOUSE_SIZES[t])


@pytest.mark.parametrize("n", cc.ONES_SIZES)
def test_ones(n):
    v, r0, s = cc.ones_case(n)
    out_of = lambda f, ab: cc.epi(np.full(n, f[0], F32), r0, ab)
    check(f"ones {n}", np.ones((1, n), F32), v, s, out_of, lambda ab: [out_of(f, ab) for f in s.F], touched=lambda j: np.arange(n),
          teeth=teeth_of(("ones", "f32", n)))


@pytest.mark.parametrize("m,n,cplx", [(m, n, False) for m, n, _ in cc.GEMV_SHAPES] + [(m, n, True) for m, n in cc.CGEMV_SHAPES])
def test_dense(m, n, cplx):
    c = cc.dense_case(m, n, cplx)
    A = c["A"]
    for mode, W in (("N", A), ("T", A.T)) + ((("C", np.conj(A.T)),) if cplx else ()):
        x, r0, s = c[mode]
        E = cc.epi_of(cplx)
        check(f"dense {'c64' if cplx else 'f32'} {m} x {n} {mode}", W, x, s, lambda f, ab: E(f, r0, ab), lambda ab: [E(f, r0, ab) for f in s.F])
        for col in (1, 8):                                  # a block column: the operand scaled by 2^-col
            sc = s.scale(-col)
            xs = x * F32(2.0 ** -col)
            ok = cc.member(E(acc64(W, xs), r0, (2.0, -3.0)), [E(f, r0, (2.0, -3.0)) for f in sc.F])
            assert ok.all(), ("scaled column", m, n, mode, col)


@pytest.mark.parametrize("t,n", [(t, n) for t in ("f32", "c64") for n in cc.HERM_SIZES])
def test_hermitian(t, n):
    c = cc.herm_case(t, n)
    cplx = t == "c64"
    d, L, v, r0, s1, s2 = (c[k] for k in ("d", "L", "v", "r0", "s1", "s2"))
    assert np.array_equal(np.triu(L), np.zeros_like(L))
    LH = np.conj(L.T)
    E = cc.epi_of(cplx)
    cands_of = lambda ab: cc.herm_candidates(t, n, ab)
    f1, f2 = acc64(L, v), acc64(LH, v)
    # teeth of either sum on its own: the other one from the Float64 model (row 0 of L and the last column are empty)
    check(f"hermitian {t} {n} L v", L, v, s1, lambda f, ab: E(cc.herm_inner(d, v, f, f2, cplx), r0, ab), cands_of)
    check(f"hermitian {t} {n} L' v", LH, v, s2, lambda f, ab: E(cc.herm_inner(d, v, f1, f, cplx), r0, ab), cands_of)
    for col in range(1, cc.HERM_K):
        vs = v * F32(2.0 ** -col)
        out = E(cc.herm_inner(d, vs, acc64(L, vs), acc64(LH, vs), cplx), np.roll(r0, col), (2.0, -3.0))
        assert cc.member(out, cc.herm_candidates(t, n, (2.0, -3.0), col)).all(), ("scaled column", t, n, col)


@pytest.mark.parametrize("chunks,long_row", cc.SPARSE_SHAPES)
def test_sparse(chunks, long_row):
    c = cc.sparse_case(chunks, long_row)
    A = c["A"]
    assert A.dtype == F32 and (np.diff(A.tocsr().indptr)[:128 * (chunks - (3 if long_row else 0))] == 16).all()
    for mode, M in (("N", A.tocsr()), ("T", A.T.tocsr())):
        x, r0, s = c[mode]
        name = f"sparse {chunks} {long_row} {mode}"
        assert s.sizes.max() <= 2, name
        print(f"{name}: cancellation ratio S_i / |y_i| median {s.ratio:.0f}, worst {s.ratio_max:.0f}, terms {s.terms}, largest |F_i| {int(s.sizes.max())}")
        M64 = M.astype(np.float64)
        for ab in cc.SCALARS:
            cands = [cc.epi(f, r0, ab) for f in s.F]
            assert cc.member(cc.epi((M64 @ x.astype(np.float64)).astype(F32), r0, ab), cands).all(), (name, ab, "Float64 model outside")
            if ab == cc.SCALARS[2]:
                continue
            assert not cc.member(cc.epi(M @ x, r0, ab), cands).all(), (name, ab, "Float32 accumulation stays inside the set")
            j = int(M.indices[M.indices.size // 3])
            for factor in (0.0, 2.0):
                xx = x.astype(np.float64)
                xx[j] *= factor
                ok = cc.member(cc.epi((M64 @ xx).astype(F32), r0, ab), cands)
                hit = np.flatnonzero(np.asarray(abs(M[:, [j]]).sum(axis=1)).ravel() > 0)
                assert hit.size and not ok[hit].any(), (name, ab, f"term {j} x {factor}", "stays inside the set")


def test_blockdiag():
    c = cc.blockdiag_case()
    for mode in ("N", "T"):
        x, r0 = c[mode]
        for ab in cc.SCALARS:
            cands = cc.blockdiag_candidates(mode, ab)
            # the Float64 model of the whole block matrix, dense blocks only (the elementwise ones are exact in the candidates)
            out, ro, xo = cands[0].copy(), 0, 0
            for (a, b), kind in zip(c["shapes"], ("d1", "M1", "eye", "M2", "zero", "d2")):
                if mode == "T":
                    a, b = b, a
                if kind in ("M1", "M2"):
                    W = c[kind].T if mode == "T" else c[kind]
                    s = cc.sums(W, x[xo:xo + b])
                    assert s.sizes.max() <= 2
                    out[ro:ro + a] = cc.epi(acc64(W, x[xo:xo + b]), r0[ro:ro + a], ab)
                    bad = cc.epi(acc32_seq(W, x[xo:xo + b]) if b > 4 else tampered(W, x[xo:xo + b], 2.0)[0], r0[ro:ro + a], ab)
                    if ab is not None and ab[1] != 0 and isinstance(ab[0], float):
                        assert not cc.member(bad, [k[ro:ro + a] for k in cands]).all(), ("blockdiag", mode, kind, "no teeth")
                ro, xo = ro + a, xo + b
            assert cc.member(out, cands).all(), ("blockdiag", mode, ab)


def test_epilogue_matches_the_oracle_bit_for_bit():
    """epi against oracle.eye_mul (alpha * v + beta * res in the reference's mixed-precision rule)"""
    import oracle
    rng = np.random.default_rng(5)
    f, r = rng.standard_normal(4099).astype(F32), rng.standard_normal(4099).astype(F32)
    for ab in cc.SCALARS[1:] + ((np.float32(1.5), -3.0), (2.0, np.float32(0.25)), (2.0, 0.0)):
        want = oracle.eye_mul(r.copy(), f, float(ab[0]), float(ab[1]), flags=oracle.scalar_flags(F32, *ab) | oracle.TAIL_BETA)
        assert cc.bits(cc.epi(f, r, ab)).tolist() == cc.bits(want).tolist(), ab


def test_forms_are_the_values_of_the_forms_table():
    """every (key, value) run here is a value tests/forms_cases.py lists for that key"""
    for forms in cc.FORMS.values():
        for settings in forms:
            for k, v in settings.items():
                assert v in {x for r in fc.FORMS[k] for x in r["values"]} | {x for r in fc.FORMS[k] for x in [r["fixed"].get(k)]}, (k, v)
