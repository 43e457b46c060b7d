"""-m gpu: the Float32 / ComplexF32 reduction kernels against their documented arithmetic: the sum accumulated
in Float64, rounded to the element type once, then the reference's alpha, beta epilogue. The inputs cancel (|y_i| is 3000 to
11 000 times smaller than (|A||v|)_i up to a few thousand terms, 8 to 110 times at 3e5 to 4e6 terms, where a larger ratio would let
the Float64 accumulation itself move the rounded sum by more than one float: f32_contract_cases.delta_exp), the reference is exact, and the assertion is per element and on BITS: every output must
be one of the at most two (per component) values the contract allows. tests/f32_contract_cases.py builds inputs, sets and
models and says how; tests/test_f32_contract_host.py shows on the CPU that Float32 accumulation, a dropped and a doubled
term all fail this assertion.

Every family runs in the 3-argument form onto a NaN-filled res (beta = 0 never reads it), with (alpha, beta) = (2, -3) as
Float64 scalars and (1.5f0, 0.25f0) as Float32 scalars, under the default form and under every tune key of
tests/forms_cases.py that selects another kernel form for it (one case per form, inside ctx.tuned). The forms of
forms_cases.WAIVABLE may refuse on a shared card and fall back by themselves; the assertion holds for whichever form ran.

The same inputs, widened to Float64 (ComplexF64), go through the Float64 kernels against the any-order bound
(terms + R) * 2^-53 * (|alpha| S_i + |beta| |r_i|) per element (R: tests/tolerances.py, F64_CONTRACT_R). A ComplexF64 element is
16 bytes, so those operands have one 16-byte phase only. A NaN in an output fails either assertion.

test_kept_householder runs the kept-rounds dot launch of opHouseholder with none, some and all chunks of h resident
(csrc/house_keep.h), forced the way tests/test_gpu_house_keep.py and test_gpu_house_resident.py force it, at n = 4 R + 1 — the
smallest n it takes — and asserts its two launches. test_contract asserts the launch count of one apply for gemv_n_rows and
gemvb_n_rows (ENGAGED), the keys of these families whose forms change it and cannot refuse at run time.

Out of scope: kron (Float32 accumulation in the MFMA by design), the quasi-Newton applies and push! (panels of already
rounded derived columns; measured envelope in tolerances.py), krylov.hip (tests/test_gpu_opnorm.py, longdouble measure), the
factorisation operators and the sharded paths."""
import numpy as np
import pytest
import torch

import f32_contract_cases as cc
import forms_cases as fc
from test_gpu_forms import cm, counted, host, launches, place
from tolerances import F64_CONTRACT_R as R64

pytestmark = pytest.mark.gpu

LD = cc.LD
HI, FORMS = fc.HI_PER_CU, cc.FORMS
CASES = [(fam, i) for fam, forms in FORMS.items() for i in range(len(forms))]
WIDE = {np.dtype(np.float32): np.float64, np.dtype(np.complex64): np.complex128}
_DEV = {}


def form_name(settings):
    return " ".join(f"{k}={v}" for k, v in settings.items()) or "default"


def dev_once(key, make):
    """device operands of a (family, shape), uploaded once and never written"""
    if key not in _DEV:
        _DEV[key] = make()
    return _DEV[key]


def wide(a):
    return a.astype(WIDE[a.dtype])


def apply(lo, res, op, v, ab):
    if ab is None:
        lo.mul(res, op, v)
    else:
        lo.mul(res, op, v, *ab)
    return host(res)


def nan_like(r0):
    out = np.full(r0.shape, np.nan, r0.dtype)
    if np.iscomplexobj(out):
        out.imag = np.nan
    return out


def start(r0, ab):
    """res before the apply: NaN for the 3-argument form"""
    return nan_like(r0) if ab is None else r0


def in_set(got, cands, what, form, exact=None, e=None):
    ok = cc.member(got, cands)
    if ok.all():
        return
    i = tuple(int(k) for k in np.argwhere(~ok)[0])
    msg = f"{what} [{form}]: element {i} = {got[i]!r} is none of {[c[i] for c in cands]!r}; {int((~ok).sum())} of {ok.size} outside"
    parts = (np.real, np.imag) if np.iscomplexobj(got) else (np.asarray,)
    away = max(min(abs(float(p(got[i])) - float(p(c[i]))) / float(np.spacing(np.abs(p(c[i])).astype(np.float32))) for c in cands) for p in parts)
    msg += f"; {away:.3g} Float32 ulp from the nearest allowed value"
    if exact is not None:
        msg += f"; rounded sum: err / e_i = {float(abs(LD(got[i].real) - exact[i].real) / e[i].real):.3g} (alpha = 1, beta = 0 only)"
    raise AssertionError(msg)


def in_bound(got, exact, B, what, form):
    q = cc.f64_excess(got, exact, B)
    if (q <= 1).all():                                       # False for a NaN
        return
    i = int(np.argmax(~(q <= 1)))
    raise AssertionError(f"{what} [{form}]: err / B_i = {float(q[i]):.3g} at (component-stacked) index {i}")


# ------------------------------------------------------------------------------------------------ runners
def run_dots(lo, dev, ctx, form):
    """mxlo_dot / mxlo_dot_c: the device scalar is the unrounded Float64 sum — |got - y| <= e, operands at equal and mixed phases"""
    from linearoperators_jl_amd.device import dtype_code, ptr
    for t in ("f32", "c64"):
        for n in cc.DOT_SIZES[t]:
            a, b, s = cc.dot_case(t, n)
            for prec, conv in (("32", lambda z: z), ("64", wide)):
                az, bz = conv(a), conv(b)
                for offa, offb in ((0, 0), (1, 1), (0, 1)):
                    if az.dtype == np.complex128 and (offa or offb):
                        continue
                    ad, bd = place(az, offa, dev), place(bz, offb, dev)
                    out = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
                    if t == "c64":
                        lo._lib.call("mxlo_dot_c", ctx.handle, dtype_code(ad.dtype, complex_ok=True), ptr(ad), ptr(bd), n, ptr(out))
                        got = host(out)
                        err = (abs(LD(got[0]) - s.y[0].real) / s.e[0].real, abs(LD(got[1]) - s.y[0].imag) / s.e[0].imag)
                    else:
                        lo._lib.call("mxlo_dot", ctx.handle, dtype_code(ad.dtype), ptr(ad), ptr(bd), n, ptr(out))
                        got = host(out)
                        err = (abs(LD(got[0]) - s.y[0]) / s.e[0],)
                    assert max(err) <= 1, f"dot {t}/{prec} n={n} phases {offa},{offb} [{form}]: err / e = {float(max(err)):.3g}, got {got}"


def _house_f64_bound(h, v, r0, s, ab):
    """res = alpha (v - c h) + beta r, c = 2 dot: the dot's any-order error n 2^-53 S through 2 |alpha| |h_i|, and R roundings
    (c h, v - c h, alpha inner, beta r, the sum: stream_kernels.h:276-277,212) of the magnitudes they act on"""
    a, b = (1.0, 0.0) if ab is None else ab
    hl, vl, rl = h.astype(LD), v.astype(LD), r0.astype(LD)
    c = 2 * s.y[0]
    exact = LD(a) * (vl - c * hl) + (LD(b) * rl if b != 0 else 0)
    u = LD(2) ** -53
    B = abs(a) * 2 * (s.terms * u * s.S[0]) * np.abs(hl) + R64["householder"] * u * (abs(a) * (np.abs(vl) + abs(c) * np.abs(hl)) + abs(b) * np.abs(rl))
    return exact, B


def _chouse_f64_bound(h, v, r0, s, ab):
    """the complex form, per component: p = c .* h takes two products and a sum (complex.hip:101), then v - p and the three
    roundings of cfin; the dot's two errors reach a component of p through 2 (e_re |h_re| + e_im |h_im|) at most"""
    a, b = (1.0, 0.0) if ab is None else ab
    CL = np.clongdouble
    hl, vl, rl = h.astype(CL), v.astype(CL), r0.astype(CL)
    c = 2 * s.y[0]
    exact = LD(a) * (vl - c * hl) + (LD(b) * rl if b != 0 else 0)
    u = LD(2) ** -53
    ha = np.abs(hl.real) + np.abs(hl.imag)
    dot = abs(a) * 2 * max(s.e[0].real, s.e[0].imag) * ha
    mag = (abs(c.real) + abs(c.imag)) * ha
    Br = dot + R64["householder_complex"] * u * (abs(a) * (np.abs(vl.real) + mag) + abs(b) * np.abs(rl.real))
    Bi = dot + R64["householder_complex"] * u * (abs(a) * (np.abs(vl.imag) + mag) + abs(b) * np.abs(rl.imag))
    return exact, Br + 1j * Bi


def run_house(lo, dev, ctx, form):
    """opHouseholder(h) on Float32 and ComplexF32 (bits in the set) and on Float64 (bound); h and v at equal and mixed phases"""
    for t in ("f32", "c64"):
        for n in cc.HOUSE_SIZES[t]:
            h, v, r0, s = cc.house_case(t, n)
            for offh, offv in ((0, 0), (1, 1), (0, 1)):
                hd, vd = place(h, offh, dev), place(v, offv, dev)
                H = lo.opHouseholder(hd)
                for ab in cc.SCALARS:
                    got = apply(lo, place(start(r0, ab), offv, dev), H, vd, ab)
                    in_set(got, cc.house_candidates(t, n, ab), f"householder {t} n={n} phases {offh},{offv} {ab}", form)
            hd, vd = place(wide(h), 0, dev), place(wide(v), 0, dev)
            H = lo.opHouseholder(hd)
            for ab in cc.SCALARS[:2]:
                got = apply(lo, place(start(wide(r0), ab), 0, dev), H, vd, ab)
                bound = _house_f64_bound(h, v, r0, s, ab) if t == "f32" else _chouse_f64_bound(h, v, r0, s, ab)
                in_bound(got, *bound, f"householder {t}/64 n={n} {ab}", form)


def run_ones(lo, dev, ctx, form):
    for n in cc.ONES_SIZES:
        v, r0, s = cc.ones_case(n)
        for dtype, conv in ((torch.float32, lambda z: z), (torch.float64, wide)):
            O = lo.opOnes(dtype, n, n, S=lo.Storage(dtype, dev))
            for off in (0, 1):
                vd = place(conv(v), off, dev)
                for ab in cc.SCALARS:
                    got = apply(lo, place(start(conv(r0), ab), off, dev), O, vd, ab)
                    if dtype == torch.float32:
                        in_set(got, [cc.epi(np.full(n, f[0], cc.F32), r0, ab) for f in s.F], f"ones n={n} phase {off} {ab}", form)
                    elif not isinstance(ab and ab[0], np.float32):
                        full = cc.Sum(np.full(n, s.y[0]), np.full(n, s.S[0]), s.terms)
                        in_bound(got, *cc.f64_bound(full, r0, ab, R64["fin_ab"]), f"ones f64 n={n} {ab}", form)


def _dense_modes(lo, op, cplx):
    return (("N", op), ("T", op.T)) + ((("C", op.H),) if cplx else ())


def run_dense(lo, dev, ctx, form, shapes, cplx):
    """LinearOperator(M): M v, M.' u (and M^H u) on vectors; real data also on blocks of 4, 8 and 9 columns (column c is the
    operand times 2^-c, an exact scaling of the sums), even and odd leading dimensions"""
    E = cc.epi_of(cplx)
    for shape in shapes:
        m, n, pad = (shape + (0,))[:3]
        c = cc.dense_case(m, n, cplx)
        for prec, conv in (("32", lambda z: z), ("64", wide)):
            op = dev_once(("dense", m, n, cplx, prec), lambda: lo.LinearOperatorFromMatrix(cm(conv(c["A"]), pad, dev)))
            for mode, o in _dense_modes(lo, op, cplx):
                x, r0, s = c[mode]
                what = f"dense {'c' if cplx else 'f'}{prec} {m}x{n} ld+{pad} {mode}"
                for ab in cc.SCALARS if prec == "32" else cc.SCALARS[:2]:
                    got = apply(lo, place(conv(start(r0, ab)), 0, dev), o, place(conv(x), 0, dev), ab)
                    if prec == "32":
                        in_set(got, [E(f, r0, ab) for f in s.F], f"{what} {ab}", form, s.y, s.e)
                    else:
                        in_bound(got, *cc.f64_bound(s, r0, ab, R64["fin_ab"]), f"{what} {ab}", form)
                if cplx:
                    continue
                for k in cc.BLOCK_K:
                    X = np.stack([x * cc.F32(2.0 ** -j) for j in range(k)], axis=1)
                    R0 = np.stack([np.roll(r0, j) for j in range(k)], axis=1)
                    for ab in cc.SCALARS if prec == "32" else cc.SCALARS[1:2]:
                        res = cm(conv(start(R0, ab)), pad, dev)
                        if ab is None:
                            lo.mul(res, o, cm(conv(X), pad, dev))
                        else:
                            lo.mul(res, o, cm(conv(X), pad, dev), *ab)
                        got = host(res)
                        for j in range(k):
                            sj = s.scale(-j)
                            if prec == "32":
                                in_set(got[:, j], [E(f, R0[:, j], ab) for f in sj.F], f"{what} block k={k} column {j} {ab}", form, sj.y, sj.e)
                            else:
                                in_bound(got[:, j], *cc.f64_bound(s, R0[:, j], ab, R64["fin_ab"], col=j), f"{what} block k={k} column {j} {ab}", form)


def _herm_f64_bound(c, ab, cplx, col=0):
    """alpha ((d v + a1) + a2) + beta r: terms + R roundings of |d v| + S1 + S2 (dense.hip:1526-1527; complex.hip:935-938)"""
    a, b = (1.0, 0.0) if ab is None else ab
    f = LD(2.0) ** -col
    s1, s2 = c["s1"], c["s2"]
    ct = np.clongdouble if cplx else LD
    d, v, r = c["d"].astype(LD), c["v"].astype(ct) * f, np.roll(c["r0"], col).astype(ct)
    exact = LD(a) * (d * v + s1.y * f + s2.y * f) + (LD(b) * r if b != 0 else 0)
    k = LD(s1.terms + R64["hermitian"]) * LD(2) ** -53
    part = lambda z: (np.real(z), np.imag(z)) if cplx else (z,)
    Bs = [k * (abs(a) * (np.abs(d * pv) + p1 * f + p2 * f) + abs(b) * np.abs(pr)) for pv, p1, p2, pr in zip(part(v), part(s1.S), part(s2.S), part(r))]
    return exact, (Bs[0] + 1j * Bs[1] if cplx else Bs[0])


def run_herm(lo, dev, ctx, form):
    """opHermitian(d, A), real and complex with a Real d: vector and (real data) a block of 3 columns; NaN on and above the
    diagonal of A is never read"""
    for t in ("f32", "c64"):
        cplx = t == "c64"
        for n in cc.HERM_SIZES:
            c = cc.herm_case(t, n)
            for prec, conv in (("32", lambda z: z), ("64", wide)):
                def make():
                    Ad = conv(c["L"]).copy()
                    Ad[np.triu_indices(n)] = np.nan
                    return lo.opHermitian(torch.from_numpy(conv(c["d"])).to(dev), cm(Ad, 0, dev))
                H = dev_once(("herm", t, n, prec), make)
                vd = place(conv(c["v"]), 0, dev)
                for ab in cc.SCALARS if prec == "32" else cc.SCALARS[:2]:
                    got = apply(lo, place(conv(start(c["r0"], ab)), 0, dev), H, vd, ab)
                    if prec == "32":
                        in_set(got, cc.herm_candidates(t, n, ab), f"hermitian {t} n={n} {ab}", form)
                    else:
                        in_bound(got, *_herm_f64_bound(c, ab, cplx), f"hermitian {t}/64 n={n} {ab}", form)
                if cplx:
                    continue
                V = np.stack([c["v"] * cc.F32(2.0 ** -j) for j in range(cc.HERM_K)], axis=1)
                R0 = np.stack([np.roll(c["r0"], j) for j in range(cc.HERM_K)], axis=1)
                for ab in cc.SCALARS if prec == "32" else cc.SCALARS[1:2]:
                    res = cm(conv(start(R0, ab)), 1, dev)
                    if ab is None:
                        lo.mul(res, H, cm(conv(V), 1, dev))
                    else:
                        lo.mul(res, H, cm(conv(V), 1, dev), *ab)
                    got = host(res)
                    for j in range(cc.HERM_K):
                        if prec == "32":
                            in_set(got[:, j], cc.herm_candidates(t, n, ab, j), f"hermitian block {t} n={n} column {j} {ab}", form)
                        else:
                            in_bound(got[:, j], *_herm_f64_bound(c, ab, cplx, j), f"hermitian block f64 n={n} column {j} {ab}", form)


def run_sparse(lo, dev, ctx, form):
    """sparse LinearOperator(M), N and T, vector and a block of 3 columns (column c: the operand times 2^-c); the chunk count
    of the N apply is read back from mxlo_csc_info"""
    from test_gpu_sparse import dev_csc
    for chunks, long_row in cc.SPARSE_SHAPES:
        c = cc.sparse_case(chunks, long_row)
        for prec, dtype, conv in (("32", torch.float32, lambda z: z), ("64", torch.float64, wide)):
            op = dev_once(("sparse", chunks, long_row, prec), lambda: lo.LinearOperatorFromMatrix(dev_csc(c["A"], dev, dtype)))
            info = op._csc.info()
            assert info["chunks_n"] == chunks and info["long_rows"] == int(long_row), info
            for mode, o in (("N", op), ("T", lo.transpose(op))):
                x, r0, s = c[mode]
                what = f"sparse f{prec} chunks={chunks} long={long_row} {mode}"
                X = np.stack([x * cc.F32(2.0 ** -j) for j in range(3)], axis=1)
                R0 = np.stack([np.roll(r0, j) for j in range(3)], axis=1)
                for ab in cc.SCALARS if prec == "32" else cc.SCALARS[:2]:
                    got = apply(lo, place(conv(start(r0, ab)), 0, dev), o, place(conv(x), 0, dev), ab)
                    res = cm(conv(start(R0, ab)), 1, dev)
                    if ab is None:
                        lo.mul(res, o, cm(conv(X), 1, dev))
                    else:
                        lo.mul(res, o, cm(conv(X), 1, dev), *ab)
                    gotb = host(res)
                    if prec == "32":
                        in_set(got, [cc.epi(f, r0, ab) for f in s.F], f"{what} {ab}", form, s.y, s.e)
                        for j in range(3):
                            sj = s.scale(-j)
                            in_set(gotb[:, j], [cc.epi(f, R0[:, j], ab) for f in sj.F], f"{what} block column {j} {ab}", form, sj.y, sj.e)
                    else:
                        in_bound(got, *cc.f64_bound(s, r0, ab, R64["fin_ab"]), f"{what} {ab}", form)
                        for j in range(3):
                            in_bound(gotb[:, j], *cc.f64_bound(s, R0[:, j], ab, R64["fin_ab"], col=j), f"{what} block column {j} {ab}", form)


def run_blockdiag(lo, dev, ctx, form):
    """the fused BlockDiagonalOperator of test_gpu_forms.run_blockdiag with cancelling dense blocks: Float32 bits in the set,
    Float64 against the bound of the whole block matrix (terms: the 300 rows of the taller dense block)"""
    c = cc.blockdiag_case()
    for prec, dtype, conv in (("32", torch.float32, lambda z: z), ("64", torch.float64, wide)):
        S = lo.Storage(dtype, dev)

        def make():
            ops = [lo.opDiagonal(place(conv(c["d1"]), 0, dev)), cm(conv(c["M1"]), 0, dev), lo.opEye(dtype, 3, S=S),
                   lo.LinearOperatorFromMatrix(cm(conv(c["M2"]), 0, dev)), lo.opZeros(dtype, 2, 5, S=S), lo.opDiagonal(place(conv(c["d2"]), 0, dev))]
            BD = lo.BlockDiagonalOperator(*ops)
            assert hasattr(BD, "_keepalive")                   # the single-launch path
            return BD
        BD = dev_once(("blockdiag", prec), make)
        for mode, o in (("N", BD), ("T", BD.T)):
            x, r0 = c[mode]
            for ab in cc.SCALARS if prec == "32" else cc.SCALARS[:2]:
                got = apply(lo, place(conv(start(r0, ab)), 0, dev), o, place(conv(x), 0, dev), ab)
                if prec == "32":
                    in_set(got, cc.blockdiag_candidates(mode, ab), f"blockdiag {mode} {ab}", form)
                else:
                    in_bound(got, *cc.f64_bound(cc.blockdiag_sums(mode), r0, ab, R64["fin_ab"]), f"blockdiag f64 {mode} {ab}", form)


RUNNERS = {"dots": run_dots, "house": run_house, "ones": run_ones,
           "gemv": lambda lo, dev, ctx, form: run_dense(lo, dev, ctx, form, cc.GEMV_SHAPES, False),
           "cgemv": lambda lo, dev, ctx, form: run_dense(lo, dev, ctx, form, cc.CGEMV_SHAPES, True),
           "herm": run_herm, "sparse": run_sparse, "blockdiag": run_blockdiag}


@pytest.mark.parametrize("family,index", CASES, ids=[f"{fam}-{form_name(FORMS[fam][i]).replace(HI, 'hi').replace(' ', ',')}" for fam, i in CASES])
def test_contract(lo, dev, family, index):
    ctx = lo.get_ctx(dev)
    table = {k: (d, lo_, hi) for k, d, lo_, hi in lo._lib.tune_keys()}
    defaults = {k: d for k, (d, _, _) in table.items()}
    assert {k: ctx.tune_get(k) for k in table} == defaults, "an earlier test left a key set"
    settings = {k: (table[k][2] // ctx.info()["num_cu"] if v == HI else v) for k, v in FORMS[family][index].items()}
    with ctx.tuned(**settings):
        RUNNERS[family](lo, dev, ctx, form_name(settings))
        torch.cuda.synchronize()
        if family == "gemv" and len(settings) == 1:
            engaged(lo, dev, ctx, *next(iter(settings.items())))
    assert {k: ctx.tune_get(k) for k in table} == defaults, "keys after the block"


# launches of one apply at the Float32 band shape of forms_cases.GEMV (8196 x 1024): M v for gemv_n_rows — one where the row
# bands run (32 / 64 / 128 rows are band heights of Float32, dense.hip:391; `auto` takes them at m >= 8 V x 256 CUs,
# dense.hip:392-397), two (partials + finish) in the column-chunk schedule — and M V with 4 columns for gemvb_n_rows
# (dense.hip:977-1018); the counts forms_cases.FORMS gives for the Float64 probe
ENGAGED = {"gemv_n_rows": {0: 2, 1: 1, 32: 1, 64: 1, 128: 1}, "gemvb_n_rows": {0: 2, 1: 1}}


def engaged(lo, dev, ctx, key, value):
    if key not in ENGAGED or (key == "gemv_n_rows" and value == 1 and ctx.info()["num_cu"] != 256):
        return
    m, n, pad = cc.GEMV_SHAPES[-1]
    c = cc.dense_case(m, n, False)
    op = dev_once(("dense", m, n, False, "32"), lambda: lo.LinearOperatorFromMatrix(cm(c["A"], pad, dev)))
    x, r0, _ = c["N"]
    k = 1 if key == "gemv_n_rows" else 4
    if k == 1:
        res, xd = place(r0, 0, dev), place(x, 0, dev)
    else:
        res, xd = cm(np.stack([r0] * k, axis=1), pad, dev), cm(np.stack([x] * k, axis=1), pad, dev)
    got = counted(lo, lambda: lo.mul(res, op, xd, 2.0, -3.0))
    assert got == ENGAGED[key][value], (key, value, "launches of one apply", got, ENGAGED[key][value])


@pytest.mark.parametrize("case", cc.KEPT_CASES)
def test_kept_householder(lo, dev, case):
    """the kept-rounds dot launch (its own workgroups exchange the partial sums and apply the c = 2 dot tail to the kept rounds)
    with none / some / all chunks of h resident: two launches, every element's bits in the set; h, v and res at both phases"""
    ctx = lo.get_ctx(dev)
    n = cc.kept_n(ctx.info()["num_cu"], 4)
    h, v, r0, s = cc.house_case("f32", n)
    settings = dict(cc.KEPT_FORCE, nt_min_bytes=cc.kept_nt_min(case, 4 * n))
    for off in (0, 1):
        hd, vd = place(h, off, dev), place(v, off, dev)
        H = lo.opHouseholder(hd)
        for ab in cc.SCALARS:
            res = place(start(r0, ab), off, dev)
            with ctx.tuned(**settings):
                l0 = launches(lo)
                got = apply(lo, res, H, vd, ab)
                assert launches(lo) - l0 == 2, ("the kept form did not run", case, off, ab, launches(lo) - l0)
            in_set(got, cc.house_candidates("f32", n, ab), f"kept householder n={n} phase {off} {ab}", f"{case} {form_name(settings)}")
    if case != "q0":
        return
    n = cc.kept_n(ctx.info()["num_cu"], 8)                    # Float64: two elements a vector, the same inputs widened
    h, v, r0, s = cc.house_case("f32", n)
    hd, vd = place(wide(h), 0, dev), place(wide(v), 0, dev)
    H = lo.opHouseholder(hd)
    for ab in cc.SCALARS[:2]:
        res = place(start(wide(r0), ab), 0, dev)
        with ctx.tuned(**settings):
            l0 = launches(lo)
            got = apply(lo, res, H, vd, ab)
            assert launches(lo) - l0 == 2, ("the kept form did not run", "f64", ab, launches(lo) - l0)
        in_bound(got, *_house_f64_bound(h, v, r0, s, ab), f"kept householder f64 n={n} {ab}", f"q0 {form_name(settings)}")
