"""Inputs, exact references and bit-level models behind test_f32_contract_host.py (CPU) and test_gpu_f32_contract.py (device).
Plain NumPy; nothing here touches a GPU.

Contract under test (csrc/reductions.hip:5, csrc/complex.hip:109,240,650): a reduction on Float32 / ComplexF32
data is accumulated in Float64, in a fixed order, rounded to the element type ONCE, and then goes through the reference's
`alpha * y + beta * res` epilogue in the caller's scalar types.

Cancelling inputs. The reduced index comes in pairs: the matrix entries of a pair are (+a, -a), the operand's are x and
fl32(x * (1 + delta)), delta = 2^-kj with kj in {k - 2, k - 1, k}; signs (phases, for complex data) are chosen so that all the
pair contributions -delta * a * x of one output element point the same way. So |y_i| is about 2^(k-1) .. 2^(k+1) times
smaller than S_i = (|A||v|)_i and every value is an exact Float32. k = min(12, 26 - ceil(log2(terms))) (`delta_exp`) keeps
2 e_i below half a Float32 ulp of y_i, so the set below never holds more than two adjacent floats. k therefore shrinks with
the number of terms: the ratio S_i / |y_i| is 3000 .. 11 000 up to a few thousand terms (k = 12), about 110 at 300 001 terms,
56 at 2^20, 16 .. 30 for the complex dots of those lengths, 8 for the 4.2 M-element kept Householder shape (k = 3); single
elements of the sparse transposed apply, whose column holds one pair, reach 10^6 .. 10^7 (test_f32_contract_host.py prints the
median and the worst ratio of every case). An odd length leaves one
unpaired element, scaled by 2^-k so that it does not drown the cancelled sum. The matrices are paired along BOTH indices
(a 2 x 2 pattern [[b, -b], [-b, b]] under a row and a column permutation), so one matrix serves M v, M' u and M^H u.

Reference. y and S are evaluated in numpy.longdouble (x87 extended, 64-bit significand — asserted below): a product of two
Float32 values is exact there, the sum carries at most terms * 2^-64 * S_i, and that is added to e_i.

The contract as a set. e_i = terms * 2^-53 * S_i (the any-order bound on the Float64 accumulation) + terms * 2^-64 * S_i
(the reference). The device's rounded sum must be in F_i = {RN32(y_i - e_i), RN32(y_i + e_i)} (`fset`), and its output in
{epi(f) : f in F_i}: `epi` restates stream_kernels.h:207-214 (fin_ab) / complex_scalars.h:15-31 (cfin) in NumPy. The library
is built with -ffp-contract=off (csrc/Makefile:2), so NumPy's separately rounded operations are the kernel's. Every Float32
kernel in scope could be modelled to the bit; the fallback bound of a norm-like tolerance is not used anywhere.

Kernel tails, as read from the code:
  dense / sparse / blockdiag   fin_ab(alpha * (CA)(T)acc, beta, old)      dense.hip:238,307,377,585,738,829,940;
                                                                          sparse_kernels.h:141; blockdiag.hip:226,238
  complex dense                t = ((R)re, (R)im); a.mul(t); cfin          complex.hip:315-321,399-405,558-559
  opOnes                       as = a * (CA)(T)sum                         stream_kernels.h:264
  opHouseholder                c = (T)2 * (T)dot; inner = v - (c * h)      stream_kernels.h:274-277,298-302; leaves.hip:286
  complex opHouseholder        cr = (R)2 * (R)dot[0], ci likewise; p = c .* h in R; inner = v - p      complex.hip:97-102
  opHermitian                  inner = ((d_i * v_i) + (T)a1) + (T)a2 with a1 = (L v)_i, a2 = (L' v)_i accumulated and rounded
                               SEPARATELY (two sets, four candidates)      dense.hip:1526; complex.hip:636,935
A Real scalar next to complex data multiplies component by component (complex_scalars.h:38-47), so with the Real
(alpha, beta) used here the complex epilogue is the real one on each component; the 3-argument form passes one(T) = 1 + 0i,
whose product with a finite t is t.

Float64 data (the same values, widened): |got_i - exact_i| <= (terms + R) * 2^-53 * (|alpha| S_i + |beta| |r_i|), the
any-order bound; R (tests/tolerances.py: F64_CONTRACT_R) counts the Float64 roundings after the sum.

Out of scope: kron (its Float32 GEMMs accumulate in Float32 in the MFMA by design), the quasi-Newton applies and push! (their
panels hold derived columns already rounded to Float32: tolerances.py has their measured envelope), krylov.hip (held to a
longdouble measure by tests/test_gpu_opnorm.py), the factorisation operators and the sharded paths.

The kept-rounds dot launch and its resident slice of h (csrc/house_keep.h) need more than four rounds of the dot launch,
n > 4 R with R = 1024 x (number of CUs) vectors; tests/test_gpu_house_keep.py and test_gpu_house_resident.py force them there
with house_fused = 1, house_inline_n = 0, house_fused_per_cu = 1 and nt_min_bytes at 0, 2/3 and 3/2 of the bytes of h (no, some
and all chunks of h resident). `kept_n` / `kept_nt_min` restate that; the Float32 shape is n = 4 R + 1 (4.2 M elements on
256 CUs), the smallest the form takes.
"""
import functools
import itertools
import math

import numpy as np
import scipy.sparse as sp

import forms_cases as fc

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs a 64-bit significand (x87 extended precision)"

F32, C64 = np.float32, np.complex64
# (alpha, beta) as the caller passes them: None is the 3-argument form (one(T), zero(T): res is never read and starts as NaN),
# Python floats are Julia Float64 scalars, numpy.float32 are Float32 scalars
SCALARS = (None, (2.0, -3.0), (np.float32(1.5), np.float32(0.25)))


# ------------------------------------------------------------------------------------------------ the forms
# per family: the settings of ctx.tuned, {} being the default form; keys and values are those of forms_cases.FORMS
HI = fc.HI_PER_CU
_SPLIT = dict(house_fused=0)
_THREE = dict(house_fused=0, house_inline_n=0)
FORMS = {
    "dots": [{}, dict(red_blocks_per_cu=1), dict(red_blocks_per_cu=4), dict(red_blocks_per_cu=HI), dict(fuse_finalize=0), dict(fuse_finalize=1),
             dict(nt_min_bytes=0)],
    "house": [{}, _SPLIT, dict(house_fused=1), _THREE, dict(house_fused_per_cu=1), dict(house_fused_per_cu=2),
              dict(_SPLIT, red_blocks_per_cu=1), dict(_SPLIT, red_blocks_per_cu=HI), dict(_THREE, red_blocks_per_cu=1),
              dict(_THREE, red_blocks_per_cu=HI), dict(_THREE, fuse_finalize=0), dict(_THREE, fuse_finalize=1), dict(_THREE, nt_min_bytes=0)],
    "ones": [{}, dict(red_blocks_per_cu=1), dict(red_blocks_per_cu=HI), dict(fuse_finalize=0), dict(fuse_finalize=1)],
    "gemv": [{}, dict(nt_min_bytes=0), dict(gemv_n_rows=0), dict(gemv_n_rows=1), dict(gemv_n_rows=32), dict(gemv_n_rows=64), dict(gemv_n_rows=128),
             dict(nt_min_bytes=0, gemv_n_rows=32), dict(gemvb_n_rows=0), dict(gemvb_n_rows=1), dict(gemvb_t_lds=0), dict(gemvb_t_lds=1)],
    "cgemv": [{}, dict(nt_min_bytes=0), dict(gemv_n_rows=0), dict(gemv_n_rows=1)],
    "herm": [{}, dict(herm_single=0), dict(herm_single=1), dict(herm_strip=1), dict(herm_strip=2), dict(herm_strip=8), dict(herm_order=0),
             dict(herm_order=1), dict(herm_single=0, herm_order=1), dict(cherm_two_pass=0), dict(cherm_two_pass=1)],
    "sparse": [{}, dict(sp_xcds=1), dict(sp_xcds=8)],
    "blockdiag": [{}, dict(nt_min_bytes=0)],
}


# ------------------------------------------------------------------------------------------------ the epilogue
def _ct(s):
    return np.float64 if isinstance(s, float) else np.float32


def epi(f, r, ab):
    """fin_ab (stream_kernels.h:207-214) after t = alpha * (CA)f: Float32 arrays f (the rounded sum) and r (old res)"""
    if ab is None:
        return f.astype(F32)                                   # 1f0 * f, beta == 0
    a, b = ab
    CA, CB = _ct(a), _ct(b)
    t = CA(a) * f.astype(CA)
    if b == 0:
        return t.astype(F32)
    P = np.float64 if np.float64 in (CA, CB) else np.float32
    return (t.astype(P) + (CB(b) * r.astype(CB)).astype(P)).astype(F32)


def cepi(f, r, ab):
    """cfin (complex_scalars.h:15-31) with Real scalars: the real epilogue on each component"""
    out = np.empty(f.shape, C64)
    out.real = epi(np.ascontiguousarray(f.real), np.ascontiguousarray(r.real), ab)
    out.imag = epi(np.ascontiguousarray(f.imag), np.ascontiguousarray(r.imag), ab)
    return out


def epi_of(cplx):
    return cepi if cplx else epi


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == C64 else a.view(np.uint32)


def member(got, cands):
    """per element: do the bits of got equal those of one candidate?"""
    g = bits(got)
    ok = np.zeros(g.shape, bool)
    for c in cands:
        ok |= g == bits(c)
    return ok


# ------------------------------------------------------------------------------------------------ sets
def delta_exp(terms):
    """k: terms * 2^k <= 2^26, so 2 e <= 2^-25 |y| (|y| >= 2^-(k+1) S): below half an ulp of y, F holds <= 2 adjacent floats"""
    return int(min(12, 26 - math.ceil(math.log2(max(terms, 2)))))


def err_bound(terms, S):
    return LD(terms) * (LD(2) ** -53 + LD(2) ** -64) * S


def fset(y, e):
    """(lo, hi) Float32: RN32(y - e), RN32(y + e), longdouble in"""
    return (y - e).astype(F32), (y + e).astype(F32)


def fset_size(lo, hi):
    """number of floats in [lo, hi]: 1 where equal, 2 where adjacent, 3 (= too many) otherwise"""
    nxt = np.nextafter(lo, np.float32(np.inf))
    return np.where(lo == hi, 1, np.where(nxt == hi, 2, 3))


class Sum:
    """one family of exact sums: y, S (longdouble, real or one per component), terms per sum"""

    def __init__(self, y, S, terms):
        self.cplx = np.iscomplexobj(y)
        self.y, self.S, self.terms = y, S, terms
        if self.cplx:
            self.e = err_bound(terms, S.real) + 1j * err_bound(terms, S.imag)
            lr, hr = fset(y.real, self.e.real)
            li, hi = fset(y.imag, self.e.imag)
            self.sizes = np.maximum(fset_size(lr, hr), fset_size(li, hi))
            self.F = [(a + 1j * b).astype(C64) for a, b in itertools.product((lr, hr), (li, hi))]
        else:
            self.e = err_bound(terms, S)
            lo, hi = fset(y, self.e)
            self.sizes = fset_size(lo, hi)
            self.F = [lo, hi]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.abs(S.real) / np.abs(y.real) if self.cplx else S / np.abs(y)
        ratio = np.asarray(ratio, dtype=np.float64)
        self.ratio = float(np.median(ratio[np.isfinite(ratio)])) if np.isfinite(ratio).any() else 0.0
        self.ratio_max = float(ratio[np.isfinite(ratio)].max()) if np.isfinite(ratio).any() else 0.0

    def scale(self, p):
        """the sums of the operand scaled by 2^p (exact): a column of a block"""
        out = Sum.__new__(Sum)
        f = np.float32(2.0) ** p
        out.cplx, out.terms, out.sizes, out.ratio, out.ratio_max = self.cplx, self.terms, self.sizes, self.ratio, self.ratio_max
        out.y, out.S, out.e = self.y * LD(f), self.S * LD(f), self.e * LD(f)
        out.F = [c * f for c in self.F]
        return out


def _exact(W, x):
    """y = W x and S = |W||x| in longdouble; complex: per component, S.real for the real part, S.imag for the imaginary"""
    if not np.iscomplexobj(W):
        Wl, xl = W.astype(LD), x.astype(LD)
        return Wl @ xl, np.abs(Wl) @ np.abs(xl)
    Wr, Wi, xr, xi = W.real.astype(LD), W.imag.astype(LD), x.real.astype(LD), x.imag.astype(LD)
    y = (Wr @ xr - Wi @ xi) + 1j * (Wr @ xi + Wi @ xr)
    S = (np.abs(Wr) @ np.abs(xr) + np.abs(Wi) @ np.abs(xi)) + 1j * (np.abs(Wr) @ np.abs(xi) + np.abs(Wi) @ np.abs(xr))
    return y, S


def sums(W, x):
    W = np.atleast_2d(W)
    cplx = np.iscomplexobj(W)
    y, S = _exact(W, x)
    return Sum(y, S, (2 if cplx else 1) * W.shape[1])


# ------------------------------------------------------------------------------------------------ inputs
def _phase(rng, n):
    """angles at least pi / 8 away from every axis: both components of exp(i phase) carry weight"""
    return rng.integers(0, 4, n) * (np.pi / 2) + rng.uniform(np.pi / 8, 3 * np.pi / 8, n)


def _pair_operand(rng, base, n, k):
    """x of length n from the ceil(n / 2) base values: x[2q] = base[q], x[2q + 1] = fl32(base[q] * (1 + 2^-kj))"""
    ct = base.dtype
    x = np.empty(n, ct)
    x[0::2] = base
    h = n // 2
    kj = rng.integers(max(k - 2, 1), k + 1, h)
    x[1::2] = (base[:h].astype(np.complex128 if ct == C64 else np.float64) * (1.0 + 2.0 ** -kj)).astype(ct)
    return x


@functools.lru_cache(maxsize=None)
def paired(m, n, cplx=False, seed=0, pair_rows=True, permute=True):
    """dict(A, x, u, uc): A (m x n, Float32 or ComplexF32) paired along its columns for A x and (pair_rows) along its rows
    for A' u (real or complex transpose) and A^H uc. Everything read-only."""
    rng = np.random.default_rng(7000 + 31 * m + n + 1000003 * seed + (17 if cplx else 0))
    ct = C64 if cplx else F32
    w = 4 if cplx else 1                                     # complex: two products per term, |cos|, |sin| >= 0.38
    kn, km = delta_exp(w * n), delta_exp(w * m)
    bm, bn = ((m + 1) // 2 if pair_rows else m), (n + 1) // 2
    mag, xm, um = rng.uniform(0.5, 1, (bm, bn)), rng.uniform(0.5, 1, bn), rng.uniform(0.5, 1, bm)
    if cplx:
        tau, sig = _phase(rng, bm), _phase(rng, bn)
        B = mag * np.exp(1j * (tau[:, None] - sig[None, :]))   # B x: phase tau_i; B.' u: phase -sig_j; B^H uc: phase sig_j
        xb, ub = xm * np.exp(1j * sig), um * np.exp(-1j * tau)
    else:
        t, s = rng.choice([-1.0, 1.0], bm), rng.choice([-1.0, 1.0], bn)
        B = mag * t[:, None] * s[None, :]
        xb, ub = xm * s, um * t
    B, xb, ub = B.astype(ct), xb.astype(ct), ub.astype(ct)
    hn = n // 2
    A = np.empty((m, n), ct)
    if pair_rows:
        hm = m // 2
        A[0::2, 0::2] = B
        A[0::2, 1::2] = -B[:, :hn]
        A[1::2, 0::2] = -B[:hm, :]
        A[1::2, 1::2] = B[:hm, :hn]
        if m % 2:
            A[m - 1, :] *= ct(2.0 ** -km)
    else:
        A[:, 0::2] = B
        A[:, 1::2] = -B[:, :hn]
    if n % 2:
        A[:, n - 1] *= ct(2.0 ** -kn)
    x = _pair_operand(rng, xb, n, kn)
    if pair_rows:
        u, uc = _pair_operand(rng, ub, m, km), None
        if cplx:
            uc = np.conj(u)                                  # the same pairs, phases mirrored
    else:
        u = uc = None
    if permute:
        pc = rng.permutation(n)
        A, x = A[:, pc], x[pc]
        if pair_rows:
            pr = rng.permutation(m)
            A, u = A[pr, :], u[pr]
            uc = uc[pr] if uc is not None else None
    out = dict(A=np.ascontiguousarray(A), x=x, u=u, uc=uc)
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


def res0(rng, shape, cplx, scale):
    """old contents of res: uniform(-1, 1) times a power of two near `scale` — of the size of y, so that beta * res does not
    bury alpha * y"""
    p = np.float32(2.0) ** int(np.round(np.log2(float(scale)))) if scale > 0 and np.isfinite(scale) else np.float32(1)
    r = rng.uniform(-1, 1, shape).astype(F32)
    if cplx:
        r = (r + 1j * rng.uniform(-1, 1, shape).astype(F32)).astype(C64)
    return r * p


def _scale_of(s):
    a = np.abs(np.asarray(s.y, dtype=np.complex128 if s.cplx else np.float64))
    a = a[a > 0]
    return float(np.median(a)) if a.size else 1.0


def _ro(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs if len(arrs) > 1 else arrs[0]


# ---- dots
# forms_cases.DOTS on 4-byte components; a ComplexF32 element is 8 bytes (V = 2): its own 4V - 1 = 7 and 4V = 8 come first
DOT_SIZES = {"f32": fc.red_sizes("f32") + [1 << 20], "c64": [7, 8] + fc.red_sizes("f32") + [1 << 20]}


@functools.lru_cache(maxsize=None)
def dot_case(t, n):
    """(a, b, Sum): mxlo_dot(a, b) = sum a_i b_i, mxlo_dot_c(a, b) = sum conj(a_i) b_i"""
    cplx = t == "c64"
    p = paired(1, n, cplx, seed=1, pair_rows=False)
    W, x = p["A"], p["x"]
    a = np.conj(W[0]) if cplx else W[0].copy()
    return _ro(a, x) + (sums(W, x),)


# ---- opHouseholder, opOnes
HOUSE_SIZES = {"f32": fc.red_sizes("f32"), "c64": [7, 8] + fc.red_sizes("f32")}    # forms_cases.HOUSE; 4V - 1, 4V of both element sizes
ONES_SIZES = fc.red_sizes("f32")
# edge only — the shapes stay in the GPU test for their raggedness, the host test asserts `inside` there and not the teeth:
#   Householder: a handful of pairs whose dot rounds into c * h far below an ulp of v for most elements; teeth at 4099, 300 001
#   opOnes 15, 16: a Float32 sum of eight pairs is exact more often than not, so the Float32-ACCUMULATION teeth are off; the
#   dropped and the doubled term are still asserted
#   mxlo_dot_c 7, 8: three or four pairs — as opOnes
EDGE_ONLY = {("house", t, n) for t in ("f32", "c64") for n in (7, 8, 15, 16)} | {("ones", "f32", 15), ("ones", "f32", 16)} | \
            {("dot", "c64", 7), ("dot", "c64", 8)}
TAMPER_ONLY = {c for c in EDGE_ONLY if c[0] != "house"}       # edge only for the accumulation; a lost or doubled term must show


def kept_n(num_cu, esize=4):
    """4 R + 1: the smallest n the kept form of the Householder dot launch takes (tests/test_gpu_house_keep.py:38-42)"""
    return 4 * num_cu * 1024 * (16 // esize) + 1


def kept_nt_min(case, h_bytes):
    """nt_min_bytes that leaves none / some / all of h's chunks resident (tests/test_gpu_house_resident.py:46-48)"""
    return {"q0": 0, "qmid": h_bytes * 2 // 3, "q16": h_bytes * 3 // 2}[case]


KEPT_FORCE = dict(house_fused=1, house_inline_n=0, house_fused_per_cu=1)
KEPT_CASES = ("q0", "qmid", "q16")


def house_model(h, v, f, cplx):
    """inner for a rounded dot f (one value): stream_kernels.h:274-277 / complex.hip:97-102"""
    if not cplx:
        c = F32(2) * F32(f)
        return v - (c * h)
    cr, ci = F32(2) * F32(f.real), F32(2) * F32(f.imag)
    hr, hi = np.ascontiguousarray(h.real), np.ascontiguousarray(h.imag)
    pr, pi = (cr * hr) - (ci * hi), (cr * hi) + (ci * hr)
    out = np.empty(h.shape, C64)
    out.real, out.imag = v.real - pr, v.imag - pi
    return out


@functools.lru_cache(maxsize=None)
def house_case(t, n):
    """(h, v, r0, Sum of dot(h, v)): res = alpha (v - 2 dot(h, v) h) + beta res, dot conjugates h"""
    cplx = t == "c64"
    p = paired(1, n, cplx, seed=2, pair_rows=False)
    W, v = p["A"], p["x"]
    h = np.conj(W[0]) if cplx else W[0].copy()
    r0 = res0(np.random.default_rng(n), n, cplx, 1.0)
    return _ro(h, v, r0) + (sums(W, v),)


def house_candidates(t, n, ab):
    h, v, r0, s = house_case(t, n)
    cplx = t == "c64"
    return [epi_of(cplx)(house_model(h, v, f[0], cplx), r0, ab) for f in s.F]


@functools.lru_cache(maxsize=None)
def ones_case(n):
    """(v, r0, Sum of sum(v)): opOnes(n, n)"""
    rng = np.random.default_rng(4000 + n)
    k = delta_exp(n)
    z = rng.uniform(0.5, 1, (n + 1) // 2).astype(F32)
    v = _pair_operand(rng, z, n, k)
    v[0::2] *= F32(-1)
    if n % 2:
        v[n - 1] *= F32(2.0 ** -k)
    v = v[rng.permutation(n)]
    s = sums(np.ones((1, n), F32), v)
    r0 = res0(rng, n, False, _scale_of(s))
    return _ro(v, r0) + (s,)


# ---- dense
GEMV_SHAPES = [s[1:] for s in fc.GEMV if s[0] == "f32"]         # (m, n, extra leading dimension)
CGEMV_SHAPES = [s[1:] for s in fc.CGEMV]
BLOCK_K = fc.GEMV_K


@functools.lru_cache(maxsize=None)
def dense_case(m, n, cplx):
    """dict: A, per mode ("N", "T" and, complex, "C") the operand, r0 and the Sum"""
    p = paired(m, n, cplx, seed=3)
    A = p["A"]
    out = dict(A=A)
    rng = np.random.default_rng(m + n)
    for mode, W, x in (("N", A, p["x"]), ("T", A.T, p["u"])) + ((("C", np.conj(A.T), p["uc"]),) if cplx else ()):
        s = sums(W, x)
        out[mode] = (x, _ro(res0(rng, W.shape[0], cplx, _scale_of(s))), s)
    return out


# ---- opHermitian
HERM_SIZES = (256, 512, 515, 1500)
HERM_K = 3


@functools.lru_cache(maxsize=None)
def herm_case(t, n):
    """dict(d, L, v, r0, s1, s2): L strictly lower (the stored triangle), a1 = L v, a2 = L^H v, both cancelling: the pairs are
    neighbours (2p, 2p + 1), the entry between the two members of a pair is zero, so every row of L and every column below
    the diagonal holds whole pairs only"""
    cplx = t == "c64"
    ct = C64 if cplx else F32
    rng = np.random.default_rng(6000 + n + (1 if cplx else 0))
    k = delta_exp((4 if cplx else 1) * n)
    b = (n + 1) // 2
    mag = np.tril(rng.uniform(0.5, 1, (b, b)), -1)
    mag = mag + mag.T
    xm = rng.uniform(0.5, 1, b)
    if cplx:
        sig = _phase(rng, b)
        B, xb = mag * np.exp(1j * (sig[:, None] - sig[None, :])), xm * np.exp(1j * sig)
    else:
        s = rng.choice([-1.0, 1.0], b)
        B, xb = mag * s[:, None] * s[None, :], xm * s
    B, xb = np.tril(B, -1).astype(ct), xb.astype(ct)
    B = B + np.conj(B.T)
    A = np.empty((2 * b, 2 * b), ct)
    A[0::2, 0::2], A[0::2, 1::2], A[1::2, 0::2], A[1::2, 1::2] = B, -B, -B, B
    A = A[:n, :n].copy()
    if n % 2:
        A[n - 1, :] *= ct(2.0 ** -k)
        A[:, n - 1] *= ct(2.0 ** -k)
    L = np.tril(A, -1)
    v = _pair_operand(rng, xb, n, k)
    s1, s2 = sums(L, v), sums(np.conj(L.T), v)
    scale = _scale_of(s1)
    d = res0(rng, n, False, scale)                           # d_i v_i of the size of the cancelled sums
    return dict(d=_ro(d), L=_ro(L), v=_ro(v), r0=_ro(res0(rng, n, cplx, scale)), s1=s1, s2=s2)


def herm_inner(d, v, f1, f2, cplx):
    """((d_i * v_i) + (T)a1) + (T)a2 in the element type (dense.hip:1526; complex.hip:636,935 with a Real d)"""
    if not cplx:
        return ((d * v) + f1) + f2
    out = np.empty(v.shape, C64)
    out.real = ((d * v.real) + f1.real) + f2.real
    out.imag = ((d * v.imag) + f1.imag) + f2.imag
    return out


def herm_candidates(t, n, ab, col=0):
    """candidates of column `col` of a block whose columns are v * 2^-col and r0 rolled by col (the vector apply is column 0)"""
    c = herm_case(t, n)
    cplx = t == "c64"
    f = np.float32(2.0) ** -col
    r0 = np.roll(c["r0"], col)
    return [epi_of(cplx)(herm_inner(c["d"], c["v"] * f, f1 * f, f2 * f, cplx), r0, ab) for f1 in c["s1"].F for f2 in c["s2"].F]


# ---- sparse
SPARSE_SHAPES = [s[1:] for s in fc.SPARSE if s[0] == "f32"] + [(1, False), (3, False), (9, True)]   # the f32 row and the
SPARSE_NCOL = 6000                                           # chunk counts of the Float64 rows, on Float32 data


@functools.lru_cache(maxsize=None)
def sparse_case(chunks, long_row):
    """the matrix of test_gpu_forms._sparse_matrix (rows of exactly 16 entries, 128 rows a chunk; with `long_row` a last row
    of 5000 entries) with paired entries: rows (2p, 2p + 1) share their 8 column pairs (j, j + 3000) with the 2 x 2 pattern
    [[b, -b], [-b, b]]; the long row is unpaired and scaled by 2^-k. dict(A (scipy CSC), N: (x, r0, Sum), T: (u, r0, Sum))"""
    rng = np.random.default_rng(8000 + chunks)
    half = SPARSE_NCOL // 2
    nbase = 64 * (chunks - (3 if long_row else 0))
    m = 2 * nbase + (1 if long_row else 0)
    kn, km = delta_exp(5000 if long_row else 16), delta_exp(64)      # a column meets far fewer than 64 rows
    t, s = rng.choice([-1.0, 1.0], nbase + 1), rng.choice([-1.0, 1.0], half)
    rows, cols, vals = [], [], []
    for p in range(nbase + (1 if long_row else 0)):
        last = p == nbase
        js = np.sort(rng.choice(half, size=2500 if last else 8, replace=False))
        b = (rng.uniform(0.5, 1, js.size) * t[p] * s[js]).astype(F32)
        if last:
            b = b * F32(2.0 ** -km)
        for dr, sr in ((0, 1.0),) if last else ((0, 1.0), (1, -1.0)):
            for dc, sc in ((0, 1.0), (half, -1.0)):
                rows.append(np.full(js.size, 2 * p + dr))
                cols.append(js + dc)
                vals.append(b * F32(sr * sc))
    A = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(m, SPARSE_NCOL), dtype=F32)
    A.sort_indices()
    xb = (rng.uniform(0.5, 1, half) * s).astype(F32)
    x = np.empty(SPARSE_NCOL, F32)
    x[:half] = xb
    x[half:] = (xb.astype(np.float64) * (1.0 + 2.0 ** -rng.integers(kn - 2, kn + 1, half))).astype(F32)
    ub = (rng.uniform(0.5, 1, nbase + 1) * t).astype(F32)
    u = _pair_operand(rng, ub[:(m + 1) // 2], m, km)
    coo = A.tocoo()
    out = dict(A=A)
    for mode, oi, ii, z, nout in (("N", coo.row, coo.col, x, m), ("T", coo.col, coo.row, u, SPARSE_NCOL)):
        prod = coo.data.astype(LD) * z[ii].astype(LD)         # exact; added one by one in longdouble
        y, S = np.zeros(nout, LD), np.zeros(nout, LD)
        np.add.at(y, oi, prod)
        np.add.at(S, oi, np.abs(prod))
        sm = Sum(y, S, max(int(np.bincount(oi, minlength=nout).max()), 1))
        out[mode] = (_ro(z), _ro(res0(rng, nout, False, _scale_of(sm))), sm)
    return out


# ---- fused BlockDiagonalOperator: the blocks of test_gpu_forms.run_blockdiag, the two dense ones paired
BLOCKDIAG_DENSE = ((4, 7), (300, 3))


@functools.lru_cache(maxsize=None)
def blockdiag_case():
    """dict(d1, d2, M1, M2, N: (x, r0), T: (x, r0), and per mode the candidates builder's pieces): diag(5), dense 4 x 7, eye(3),
    dense 300 x 3, zeros(2, 5), diag(1031)"""
    rng = np.random.default_rng(2)
    d1, d2 = rng.standard_normal(5).astype(F32), rng.standard_normal(1031).astype(F32)
    P1, P2 = paired(4, 7, False, seed=4), paired(300, 3, False, seed=5)
    shapes = [(5, 5), (4, 7), (3, 3), (300, 3), (2, 5), (1031, 1031)]
    nr, nc = sum(a for a, _ in shapes), sum(b for _, b in shapes)
    out = dict(d1=_ro(d1), d2=_ro(d2), M1=P1["A"], M2=P2["A"], shapes=shapes)
    for mode, total, key in (("N", nc, "x"), ("T", nr, "u")):
        x = rng.uniform(-1, 1, total).astype(F32)
        o = 0
        for (a, b), P in zip(shapes, (None, P1, None, P2, None, None)):
            w = b if mode == "N" else a
            if P is not None:
                x[o:o + w] = P[key]
            o += w
        r0 = res0(rng, nr if mode == "N" else nc, False, 2.0 ** -6)
        out[mode] = (_ro(x), _ro(r0))
    return out


def blockdiag_candidates(mode, ab):
    """two candidate outputs (every dense sum at the low / the high end of its set); the elementwise blocks are exact:
    diag (a * d) * v, eye a * v, zeros 0 — blockdiag.hip:60-75"""
    c = blockdiag_case()
    x, r0 = c[mode]
    T = mode == "T"
    outs = []
    for side in (0, 1):
        parts, ro, xo = [], 0, 0
        for (a, b), kind in zip(c["shapes"], ("d1", "M1", "eye", "M2", "zero", "d2")):
            if T:
                a, b = b, a
            xin, rin = x[xo:xo + b], r0[ro:ro + a]
            if kind in ("M1", "M2"):
                W = c[kind].T if T else c[kind]
                parts.append(epi(sums(W, xin).F[side], rin, ab))
            elif kind == "zero":                                 # res .= 0 | res .*= beta (blockdiag.hip:71-74)
                zb = ab is None or ab[1] == 0
                parts.append(np.zeros(a, F32) if zb else (_ct(ab[1])(ab[1]) * rin.astype(_ct(ab[1]))).astype(F32))
            elif kind == "eye":
                parts.append(epi(xin, rin, ab))
            else:
                parts.append(diag_epi(c[kind], xin, rin, ab))
            ro, xo = ro + a, xo + b
        outs.append(np.concatenate(parts))
    return outs


@functools.lru_cache(maxsize=None)
def blockdiag_sums(mode):
    """the exact sums of the whole block matrix (for the Float64 bound); terms: the longest sum of any block"""
    c = blockdiag_case()
    nr, nc = (sum(a for a, _ in c["shapes"]), sum(b for _, b in c["shapes"]))
    D = np.zeros((nr, nc), LD)
    r = k = 0
    for (a, b), blk in zip(c["shapes"], (np.diag(c["d1"]), c["M1"], np.eye(3), c["M2"], np.zeros((2, 5)), np.diag(c["d2"]))):
        D[r:r + a, k:k + b] = blk
        r, k = r + a, k + b
    W = D.T if mode == "T" else D
    xl = c[mode][0].astype(LD)
    return Sum(W @ xl, np.abs(W) @ np.abs(xl), max(max(a, b) for (a, b), kind in zip(c["shapes"], "dMeMzd") if kind == "M"))


def diag_epi(d, v, r, ab):
    """DiagOp (stream_kernels.h:223): fin_ab((a * (CA)d) * (CA)v, b, r)"""
    if ab is None:
        return (F32(1) * d) * v
    a, b = ab
    CA, CB = _ct(a), _ct(b)
    t = (CA(a) * d.astype(CA)) * v.astype(CA)
    if b == 0:
        return t.astype(F32)
    P = np.float64 if np.float64 in (CA, CB) else np.float32
    return (t.astype(P) + (CB(b) * r.astype(CB)).astype(P)).astype(F32)


# ------------------------------------------------------------------------------------------------ Float64 bound
def f64_bound(s, r0, ab, R, col=0):
    """(terms + R) * 2^-53 * (|alpha| S_i + |beta| |r_i|), per component for complex data; `exact` alongside"""
    a, b = (1.0, 0.0) if ab is None else (float(ab[0]), float(ab[1]))
    f = LD(2.0) ** -col
    y, S = s.y * f, s.S * f
    r = r0.astype(np.clongdouble if s.cplx else LD)
    exact = LD(a) * y + (LD(b) * r if b != 0 else 0)
    c = LD(s.terms + R) * LD(2) ** -53
    if s.cplx:
        B = c * (abs(a) * S.real + abs(b) * np.abs(r.real)) + 1j * (c * (abs(a) * S.imag + abs(b) * np.abs(r.imag)))
    else:
        B = c * (abs(a) * S + abs(b) * np.abs(r))
    return exact, B


def f64_excess(got, exact, B):
    """per element (complex: real parts, then imaginary parts) |got - exact| / B; 0 where error and bound both vanish"""
    d = got.astype(np.clongdouble if np.iscomplexobj(got) else LD) - exact
    with np.errstate(divide="ignore", invalid="ignore"):
        if np.iscomplexobj(got):
            q = np.concatenate([np.abs(d.real) / B.real, np.abs(d.imag) / B.imag])
        else:
            q = np.abs(d) / B
    both0 = np.concatenate([(d.real == 0) & (B.real == 0), (d.imag == 0) & (B.imag == 0)]) if np.iscomplexobj(got) else (d == 0) & (B == 0)
    return np.where(both0, 0, q)                             # 0 / 0 only; a NaN in got stays NaN and fails `q <= 1`
