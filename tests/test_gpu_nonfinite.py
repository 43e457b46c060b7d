"""-m gpu: NaN, ±Inf, signed zeros, subnormals and very large / very small magnitudes through the operators, against the
oracle.

One rule set for every comparison (`check_against_oracle`):
  * class map: the positions of NaN, of +Inf and of -Inf in the result are EXACTLY the oracle's;
  * finite positions of the reducing families: the family's existing tolerance (copied below with a pointer to the test
    that owns it) — no new numbers;
  * elementwise leaves: bit for bit (sign of zero, subnormals), NaN positions compare as "is NaN".

Input rules — they make the oracle's class map independent of the order of a summation, so a fixed-order tree on the
device and a sequential loop in the oracle must agree on it (the generators assert them, `reduction_operand`):
  * a reduction sees Infs of ONE sign only (the class is that sign's), or an explicit +Inf / -Inf pair (NaN in any order);
  * finite "large" data is at most 1e120 in magnitude for Float64 and 1e15 for Float32, finite "small" data at least
    1e-120 / 1e-15, wherever the values meet in a product that is then summed;
  * vectors in those cases are at most 2^16 long: no partial sum overflows or underflows in a Float32 or Float64
    accumulator;
  * no operator entry that multiplies an Inf is exactly zero, except in the explicit `0 * Inf` cases;
  * nothing is skipped inside these rules.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from tolerances import QN_F32

pytestmark = pytest.mark.gpu

NP = {torch.float64: np.float64, torch.float32: np.float32, torch.complex128: np.complex128, torch.complex64: np.complex64}
SENTINEL_BITS = 0x7FF8DEADBEEF0001            # the exchange slots' "empty" marker (csrc/common.h: kSlotEmpty), a NaN payload
BIG = {np.float64: 1e120, np.float32: 1e15}
SMALL = {np.float64: 1e-120, np.float32: 1e-15}
# scaled cases: the unscaled data has magnitudes in [0.5, 1], so x * BIG stays <= BIG and x * (2 * SMALL) stays >= SMALL
UP = lambda npd: npd(BIG[npd])
DOWN = lambda npd: npd(2 * SMALL[npd])


def unit_mags(rng, shape, npd):
    """random signs, magnitudes in [0.5, 1]: no zero, and room for both scale factors inside the magnitude rules."""
    return (rng.uniform(0.5, 1.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(npd)

# ---- tolerances: relative L2 over the finite positions, each from the test that covers the family on finite data
TOL_HOUSE = {np.float64: 1e-12, np.float32: 1e-5}      # test_gpu_leaves.py::test_householder_parity
TOL_CHOUSE = {np.complex128: 1e-12, np.complex64: 1e-5}
TOL_HERM = {np.float64: 1e-13, np.float32: 3e-5}       # Float32: test_gpu_ops.py::test_hermitian
TOL_GEMV = {np.float64: 1e-12, np.float32: 2e-5}       # test_gpu_ops.py::test_dense_operator
TOL_GEMV_BAND = {np.float64: 1e-12, np.float32: 3e-5}  # test_gpu_ops.py::test_dense_mul_row_band_kernel
TOL_KRON = {np.float64: 1e-12, np.float32: 3e-5}       # test_gpu_ops.py::test_kron
TOL_QN_REF = {np.float64: 1e-10, np.float32: QN_F32}   # test_gpu_qn.py::test_lbfgs_parity (reference-ordered forms)
TOL_QN_ALT = {np.float64: 1e-9, np.float32: QN_F32}    # test_gpu_qn.py::test_lbfgs_parity (two-pass / gram / compact)
TOL_SPARSE = {np.float64: 1e-13, np.float32: 2e-6}     # test_gpu_sparse.py: max abs <= TOL * (|a| (|A| |v|).max() + |b|)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def TM(a, dev):
    """column-major device matrix (what a Julia Matrix is)."""
    return torch.from_numpy(np.asfortranarray(a).T.copy()).to(dev).t()


def off1(a, dev):
    """`a` on the device as a view one element into a larger buffer (never 16-byte aligned for 4 / 8-byte elements)."""
    buf = torch.zeros(a.size + 1, dtype=torch.from_numpy(a[:0].copy()).dtype, device=dev)
    buf[1:].copy_(T(a, dev))
    return buf[1:]


def put(a, dev, off):
    return off1(a, dev) if off else T(a, dev)


def _real_view(a):
    a = np.ascontiguousarray(a)
    return a.view(a.real.dtype) if a.dtype.kind == "c" else a


def check_against_oracle(got, want, tol=None, bitwise=False, atol=None, what=""):
    """The comparison rules of this module (see the module docstring). `tol`: relative L2 over the positions where the
    oracle is finite; `atol`: max abs there (families whose existing bound is an absolute one); `bitwise`: every non-NaN
    position equal as an unsigned integer."""
    got, want = _real_view(np.asarray(got)), _real_view(np.asarray(want))
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    for name, g, w in (("NaN", np.isnan(got), np.isnan(want)), ("+Inf", got == np.inf, want == np.inf),
                       ("-Inf", got == -np.inf, want == -np.inf)):
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError(f"{what}: {name} positions differ from the oracle's at {bad.size} places, first {bad[:6]}: "
                                 f"got {got[bad[:6]]}, oracle {want[bad[:6]]}")
    if bitwise:
        u = {8: np.uint64, 4: np.uint32}[got.dtype.itemsize]
        keep = ~np.isnan(want)
        gb, wb = got.view(u)[keep], want.view(u)[keep]
        if not np.array_equal(gb, wb):
            bad = np.flatnonzero(gb != wb)
            raise AssertionError(f"{what}: {bad.size} elements differ in their bits, first {bad[:6]}: got {got[keep][bad[:6]]!r}, "
                                 f"oracle {want[keep][bad[:6]]!r}")
        return
    fin = np.isfinite(want)
    g, w = got[fin].astype(np.float64), want[fin].astype(np.float64)
    if not w.size:
        return
    if atol is not None:
        err = np.abs(g - w).max()
        assert err <= atol, f"{what}: max abs error {err:.3e} > {atol:.3e} on the finite positions"
        return
    assert tol is not None, "finite positions present: a tolerance is needed"
    sc = np.abs(w).max() or 1.0                         # (scaled: 1e120-sized data must not overflow the norm)
    nw = np.linalg.norm(w / sc)
    err = np.linalg.norm((g - w) / sc) / (nw if nw else 1.0)
    assert err <= tol, f"{what}: relative error {err:.3e} > {tol:.1e} on the {w.size} finite positions"


def reduction_operand(x, npd, scaled=False):
    """Asserts the input rules for a vector that enters a reduction; returns it."""
    r = _real_view(x)
    fin = r[np.isfinite(r) & (r != 0)]
    rdt = r.dtype.type
    if fin.size:
        assert np.abs(fin).max() <= BIG[rdt] and np.abs(fin).min() >= SMALL[rdt], "magnitude rule"
    if scaled:
        assert x.size <= 1 << 16, "scaled data: at most 2^16 elements"
    return x


def launches(lo):
    a = (C.c_int64 * 12)()
    lo._lib.call("mxlo_debug_counters", a)
    return a[10]


# what a single-launch fault switches off: named in a tuned(...) block, its exit puts them back
FUSED_ON = dict.fromkeys(("house_fused", "qn_fused_small", "qn_persist", "herm_single", "kron_fuse"), 1)


# =========================================================================== 1. elementwise real leaves, bit for bit
def special_values(npd):
    fi = np.finfo(npd)
    sub_min, sub_max = fi.smallest_subnormal, np.nextafter(fi.tiny, npd(0))
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, sub_min, -sub_min, sub_max, -sub_max, fi.tiny, -fi.tiny, fi.max, -fi.max,
                     1.5, -0.75, 3.0, 1.0 / 3.0, -1e-3], dtype=npd)


def pattern(npd, n, which, shift):
    """The fixed pattern cycled over n elements; the three operands (`which` = 0, 1, 2) walk it at different rates, so
    every pair of values meets within len(pattern)^2 elements, and `shift` moves the start (n = 1, 3 see other values)."""
    sv = special_values(npd)
    L = sv.size
    i = np.arange(n) + shift
    return sv[(i + which * (i // L) + 5 * which) % L].copy()


SCALARS = ((1.0, 0.0), (2.0, 3.0), (0.0, 1.0), (0.0, 0.0), (-1.0, 0.0), (1.0, -0.0))


def scalar_variants(npd):
    if npd == np.float64:
        return list(SCALARS)
    return [(np.float32(a), np.float32(b)) for a, b in SCALARS] + list(SCALARS)          # Float32 scalars, then Float64 ones


LEAF_FAMILIES = ("diag", "diag_rect", "eye", "ones", "zeros", "scale", "diagqn", "restrict_extend")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("family", LEAF_FAMILIES)
def test_elementwise_leaves_special_values_bit_exact(lo, dev, dtype, family):
    """opDiagonal (square, rectangular), opEye, opOnes, opZeros, `res .*= α`, a diagonal quasi-Newton apply, restriction and
    extension on ±0, ±Inf, NaN, the smallest / largest subnormal, the smallest normal, the largest finite and ordinary
    values: the oracle's bits, for aligned operands and for views one element into a buffer. α = 0 against Inf / NaN gives
    NaN, β = 0 (and β = -0.0) never reads `res` — which holds NaN here in every case."""
    from linearoperators_jl_amd import operators
    npd = NP[dtype]
    S = lo.Storage(dtype, dev)
    for n in (1, 3, 64, 257, 4099):
        for off in (0, 1):
            for k, (a, b) in enumerate(scalar_variants(npd)):
                fl = oracle.scalar_flags(npd, a, b)
                d, v, r0 = (pattern(npd, n, w, k + off) for w in range(3))
                what = (family, n, off, a, b)
                if family == "diag":
                    res = put(r0, dev, off)
                    lo.mul(res, lo.opDiagonal(put(d, dev, off)), put(v, dev, off), a, b)
                    want = oracle.diag_mul(r0.copy(), d, v, float(a), float(b), flags=fl)
                elif family == "diag_rect":                      # (n + 2) x n: the two tail rows are zeroed whatever β is
                    r0 = pattern(npd, n + 2, 2, k + off)
                    res = put(r0, dev, off)
                    lo.mul(res, lo.opDiagonal(n + 2, n, put(d, dev, off)), put(v, dev, off), a, b)
                    want = oracle.diag_mul(r0.copy(), d, v, float(a), float(b), n_min=n, flags=fl)
                elif family == "eye":
                    res = put(r0, dev, off)
                    lo.mul(res, lo.opEye(dtype, n, S=S), put(v, dev, off), a, b)
                    want = oracle.eye_mul(r0.copy(), v, float(a), float(b), flags=fl | oracle.TAIL_BETA)
                elif family == "ones":
                    # sum(v) must not depend on the order: exactly representable small values (any order gives the same
                    # bits) on even k, the special pattern (NaN, and a +Inf / -Inf pair from n = 3 on: NaN in any order) on odd k
                    exact = np.array([1.0, -2.0, 0.5, 3.0, -0.25], dtype=npd)[np.arange(n) % 5]
                    both = np.isposinf(v).any() and np.isneginf(v).any()
                    if k % 2 == 0 or not (np.isnan(v).any() or np.isinf(v).any()):
                        v = exact
                    elif not np.isnan(v).any() and not both:
                        v = np.where(np.isfinite(v), npd(1.0), v)                 # Infs of one sign: the sum is that Inf
                    res = put(r0, dev, off)
                    lo.mul(res, lo.opOnes(dtype, n, n, S=S), put(v, dev, off), a, b)
                    want = oracle.ones_mul(r0.copy(), v, float(a), float(b), flags=fl)
                elif family == "zeros":
                    res = put(r0, dev, off)
                    lo.mul(res, lo.opZeros(dtype, n, n, S=S), put(v, dev, off), a, b)
                    want = oracle.zeros_mul(r0.copy(), float(b), flags=fl)
                elif family == "scale":
                    res = put(r0, dev, off)
                    operators._scale(res, a)
                    want = oracle.scale(r0.copy(), float(a), flags=oracle.scalar_flags(npd, a, 0))
                elif family == "diagqn":
                    res = put(r0, dev, off)
                    lo.mul(res, lo.DiagonalPSB(put(d, dev, off)), put(v, dev, off), a, b)
                    want = oracle.DiagonalQN("psb", d).mul(r0.copy(), v, float(a), float(b), flags=fl)
                else:                                            # restriction / extension move bytes: NaN payloads included
                    if k >= 2:
                        continue
                    rng = np.random.default_rng(n + k)
                    idx = (rng.integers(1, n + 1, max(1, n // 2)) if k == 0 else np.flatnonzero(rng.random(n) < 0.6) + 1).astype(np.int64)
                    P = lo.opRestriction(idx, n, device=dev)
                    out = put(np.full(idx.size, 7, npd), dev, off)
                    lo.mul(out, P, put(v, dev, off))
                    u8 = lambda x: np.ascontiguousarray(x).view(np.uint8)
                    assert np.array_equal(u8(out.cpu().numpy()), u8(v[idx - 1])), what
                    back = put(r0, dev, off)
                    lo.mul(back, P.H, put(v[:idx.size].copy(), dev, off))
                    wantb = oracle.extend(np.empty(n, npd), v[:idx.size].copy(), idx)
                    assert np.array_equal(u8(back.cpu().numpy()), u8(wantb)), what
                    continue
                check_against_oracle(res.cpu().numpy(), want, bitwise=True, what=str(what))


def test_float32_subnormal_product_is_not_flushed(lo, dev):
    """opDiagonal in Float32: 1e-30 * 1e-10 stays the subnormal 1e-40 (and -0.0 * 1 stays -0.0)."""
    d = np.array([1e-30, -0.0, 1e-30], np.float32)
    v = np.array([1e-10, 1.0, -1e-10], np.float32)
    res = torch.full((3,), float("nan"), dtype=torch.float32, device=dev)
    lo.mul(res, lo.opDiagonal(T(d, dev)), T(v, dev), np.float32(1), np.float32(0))
    want = oracle.diag_mul(np.empty(3, np.float32), d, v, 1.0, 0.0)
    assert want[0] != 0 and abs(want[0]) < np.finfo(np.float32).tiny
    check_against_oracle(res.cpu().numpy(), want, bitwise=True, what="subnormal product")


# =========================================================================== 2. Householder
HOUSE_FORMS = {"single": (1, 1 << 23, (1,)), "two": (0, 1 << 23, (2,)), "three": (0, 0, (2, 3))}   # house_fused, house_inline_n, launches
HOUSE_CASES = ("nan_v", "nan_h", "inf_v", "inf_pair_v", "inf_v_zero_h", "big_v", "small_v")


def house_operands(npd, n, case, p, rng):
    """h (unit norm, no exact zero), v, and the expectation the input rules fix for the dot: see HOUSE_CASES."""
    h = rng.standard_normal(n)
    h[h == 0] = 0.5
    h = (h / np.linalg.norm(h)).astype(npd)
    v = unit_mags(rng, n, npd)
    if case == "nan_v":
        v[p] = np.nan
    elif case == "nan_h":
        h[p] = np.nan
    elif case == "inf_v":
        v[p] = np.inf                                    # the only Inf of the dot: its sign is sign(h[p])
    elif case == "inf_pair_v":
        q = (p + n // 3) % n
        q = q if q != p else (p + 1) % n
        h[p], h[q] = abs(h[p]), abs(h[q])                # +Inf*h[p] and -Inf*h[q] with h > 0: an explicit +Inf / -Inf pair
        v[p], v[q] = np.inf, -np.inf
    elif case == "inf_v_zero_h":
        h[p], v[p] = 0.0, np.inf                         # the explicit 0 * Inf case: NaN
    elif case == "big_v":
        v = (v * UP(npd)).astype(npd)
    elif case == "small_v":
        v = (v * DOWN(npd)).astype(npd)
    assert case == "inf_v_zero_h" or not (h == 0).any()
    reduction_operand(h, npd), reduction_operand(v, npd, scaled=case in ("big_v", "small_v"))
    return h, v


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("form", list(HOUSE_FORMS))
def test_householder_nonfinite_every_form(lo, dev, dtype, form):
    """mulHouseholder! (src/linalg.jl:77-83) as one, two and three launches (tune keys house_fused, house_inline_n; the
    launch count is witnessed — the separate-dot form is the shared dots pass + finalize + update, and its dots pass
    finalizes in its own launch while one workgroup covers n, so it counts 2 or 3): a NaN in v or h poisons the dot (all NaN), one +Inf in v gives ±Inf everywhere and NaN at
    its own position, a +Inf / -Inf pair and an Inf opposite h_i == 0 give all NaN, v scaled by 1e120 / 1e-120 (1e15 /
    1e-15 in Float32) stays finite and within the family's tolerance; the special element sits in the first chunk, in the
    last full chunk and in the ragged tail; β = 0 (res holds NaN) and β != 0."""
    npd = NP[dtype]
    ctx = lo.get_ctx(dev)
    fused, inline_n, nlaunch = HOUSE_FORMS[form]
    rng = np.random.default_rng(2024)
    with ctx.tuned(house_fused=fused, house_inline_n=inline_n):
        for n in (4099, 1 << 16):
            for case in HOUSE_CASES:
                for p in ((5,) if case in ("big_v", "small_v") else (5, n - 700, n - 1)):
                    h, v = house_operands(npd, n, case, p, rng)
                    r0 = rng.uniform(-1, 1, n).astype(npd)
                    H = lo.opHouseholder(T(h, dev))
                    vt = T(v, dev)
                    for a, b in ((1.0, 0.0), (2.0, -3.0)):
                        res = T(r0.copy(), dev)
                        if b == 0:
                            res.fill_(float("nan"))
                        l0 = launches(lo)
                        lo.mul(res, H, vt, a, b)
                        nl = launches(lo) - l0
                        assert nl in nlaunch, (form, n, nl)
                        fl = oracle.scalar_flags(npd, a, b)
                        want = oracle.householder_mul(r0.copy(), h, v, a, b, flags=fl)
                        check_against_oracle(res.cpu().numpy(), want, tol=TOL_HOUSE[npd], what=str((form, n, case, p, a, b)))
    ctx.sync()


@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64])
def test_complex_householder_nan_in_v(lo, dev, dtype):
    """The complex variant: a NaN (and, for ComplexF64, a NaN with the exchange's empty-slot payload) in the real part
    of one element of v makes every element NaN in both parts, single-launch and multi-launch forms."""
    npd = NP[dtype]
    ctx = lo.get_ctx(dev)
    rng = np.random.default_rng(8)
    n = 1 << 16
    h = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    h = (h / np.linalg.norm(h)).astype(npd)
    payloads = [np.nan] + ([np.array([SENTINEL_BITS], np.uint64).view(np.float64)[0]] if dtype == torch.complex128 else [])
    with ctx.tuned(fused_timeout_ms=250, **FUSED_ON):
        for pay in payloads:
            for fused in (1, 0):
                with ctx.tuned(house_fused=fused):
                    v = (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(npd)
                    _real_view(v)[2 * 4321] = pay
                    res = torch.empty(n, dtype=dtype, device=dev)
                    lo.mul(res, lo.opHouseholder(T(h, dev)), T(v, dev), 1.0, 0.0)
                    ctx.sync()
                    want = oracle.householder_mul(np.empty(n, npd), h, v, 1.0, 0.0, flags=oracle.scalar_flags(npd, 1.0, 0.0))
                    assert np.isnan(_real_view(want)).all()
                    check_against_oracle(res.cpu().numpy(), want, tol=TOL_CHOUSE[npd], what=f"complex householder fused={fused}")


# =========================================================================== 3. the sentinel payload
def sentinel_nan():
    x = np.array([SENTINEL_BITS], np.uint64).view(np.float64)[0]
    assert np.isnan(x)
    return x


def qn_pairs(rng, n, k, npd):
    out = []
    for _ in range(k):
        s = rng.uniform(-1, 1, n)
        y = s * rng.uniform(0.5, 2.0, n) + 1e-2 * rng.standard_normal(n)
        out.append((s.astype(npd), y.astype(npd)))
    return out


def make_qn(lo, dev, kind, dtype, n, mem, **kw):
    make = {"inv": lo.InverseLBFGSOperator, "fwd": lo.LBFGSOperator, "lsr1": lo.LSR1Operator}[kind]
    npd = NP[dtype]
    op = make(dtype, n, mem=mem, device=dev, **kw)
    O = oracle.LSR1(n, mem=mem, dtype=npd, **kw) if kind == "lsr1" else oracle.LBFGS(n, mem=mem, inverse=(kind == "inv"), dtype=npd, **kw)
    return op, O


def _sentinel_leg(lo, dev, apply, x_clean, pos, want_clean, tol, what):
    """One apply with the empty-slot NaN at x[pos]: returns without raising, all NaN, ONE launch; then the next ordinary
    apply on the same ctx is right and still one launch. `apply(x_tensor) -> result tensor`."""
    ctx = lo.get_ctx(dev)
    with ctx.tuned(fused_timeout_ms=250, **FUSED_ON):
        xt = T(x_clean, dev)
        apply(xt)                                        # warm: slot layouts armed for this shape
        l0 = launches(lo)
        got = apply(xt)
        assert launches(lo) - l0 == 1, f"{what}: the clean apply took {launches(lo) - l0} launches, not the one-launch form"
        check_against_oracle(got.cpu().numpy(), want_clean, tol=tol, what=what + " (clean, before)")
        xs = x_clean.copy()
        xs[pos] = sentinel_nan()
        assert xs.view(np.uint64)[pos] == SENTINEL_BITS
        l0 = launches(lo)
        got = apply(T(xs, dev))
        nl = launches(lo) - l0
        ctx.sync()                                       # a timed-out exchange is reported here
        assert nl == 1, (what, nl)
        assert bool(torch.isnan(got).all()), what + ": every element is NaN in the oracle"
        l0 = launches(lo)
        got = apply(xt)
        nl = launches(lo) - l0
        ctx.sync()
        assert nl == 1, (what, "after", nl)
        check_against_oracle(got.cpu().numpy(), want_clean, tol=tol, what=what + " (clean, after)")


def test_sentinel_payload_single_launch_householder(lo, dev):
    """A NaN whose bits are the exchange's empty-slot marker, in v: the partial that carries it is published as the
    canonical NaN, so no consumer mistakes it for "not yet published" (which would end in the exchange's timeout)."""
    rng = np.random.default_rng(31)
    n = 1 << 16
    h = rng.standard_normal(n)
    h /= np.linalg.norm(h)
    v = rng.uniform(-1, 1, n)
    H = lo.opHouseholder(T(h, dev))
    want = oracle.householder_mul(np.empty(n), h, v, 1.0, 0.0)
    vs = v.copy()
    vs[12345] = sentinel_nan()
    assert np.isnan(oracle.householder_mul(np.empty(n), h, vs, 1.0, 0.0)).all()

    def apply(xt):
        res = torch.empty(n, dtype=torch.float64, device=dev)
        lo.mul(res, H, xt, 1.0, 0.0)
        return res
    _sentinel_leg(lo, dev, apply, v, 12345, want, TOL_HOUSE[np.float64], "single-launch Householder")


@pytest.mark.parametrize("kind", ["inv", "fwd", "lsr1"])
@pytest.mark.parametrize("form", ["slice", "persist"])
def test_sentinel_payload_quasi_newton_single_launch(lo, dev, kind, form):
    """The same payload in x of the single-launch slice form (n = 20,000: 10 workgroups) and of the persistent form
    (n = 2^19, `qn_persist_min_bytes` = 0) of all three quasi-Newton operators."""
    ctx = lo.get_ctx(dev)
    rng = np.random.default_rng(5)
    n, mem = (20_000, 4) if form == "slice" else (1 << 19, 5)
    op, O = make_qn(lo, dev, kind, torch.float64, n, mem)
    for s, y in qn_pairs(rng, n, mem + 1, np.float64):
        lo.push(op, T(s, dev), T(y, dev))
        O.push(s, y)
    x = rng.uniform(-1, 1, n)
    want = O.mul(np.empty(n), x)
    xs = x.copy()
    xs[777] = sentinel_nan()
    assert np.isnan(O.mul(np.empty(n), xs)).all()

    def apply(xt):
        res = torch.empty(n, dtype=torch.float64, device=dev)
        lo.mul(res, op, xt, 1.0, 0.0)
        return res
    with ctx.tuned(**({"qn_persist_min_bytes": 0} if form == "persist" else {})):
        _sentinel_leg(lo, dev, apply, x, 777, want, TOL_QN_ALT[np.float64], f"quasi-Newton {form} form, {kind}")


def test_sentinel_payload_single_launch_hermitian(lo, dev):
    """The same payload in v of the single-launch opHermitian (n = 512, full row groups, aligned A), NaN on and above the
    diagonal of A at the same time."""
    rng = np.random.default_rng(6)
    n = 512
    A = rng.standard_normal((n, n))
    A[np.triu_indices(n)] = np.nan
    d, v = rng.standard_normal(n), rng.uniform(0.5, 1.5, n)
    H = lo.opHermitian(T(d, dev), TM(A, dev))
    want = oracle.hermitian_mul(np.empty(n), d, np.tril(A, -1), v, 1.0, 0.0)
    vs = v.copy()
    vs[100] = sentinel_nan()
    assert np.isnan(oracle.hermitian_mul(np.empty(n), d, np.tril(A, -1), vs, 1.0, 0.0)).all()

    def apply(xt):
        res = torch.empty(n, dtype=torch.float64, device=dev)
        lo.mul(res, H, xt, 1.0, 0.0)
        return res
    _sentinel_leg(lo, dev, apply, v, 100, want, TOL_HERM[np.float64], "single-launch opHermitian")


# =========================================================================== 4. quasi-Newton applies
QN_FORMS = {   # kind -> [(label, apply mode, push mode, reference-ordered?)]
    "inv": [("reforder", "reforder", None, True), ("twopass", "twopass", None, False)],
    "fwd": [("reforder", None, "reforder", True), ("gram", None, "gram", False), ("compact", None, "compact", False)],
    "lsr1": [("reforder", None, "reforder", True), ("gram", None, "gram", False)],
}
QN_SCHEDULES = (("single", 1, 1), ("four", 0, 0))       # label, qn_fused_small, qn_persist


def _qn_apply_cases(lo, dev, kind, dtype, n, mem, schedules, scaled=True):
    npd = NP[dtype]
    ctx = lo.get_ctx(dev)
    rng = np.random.default_rng(n + 31 * mem)
    prs = qn_pairs(rng, n, mem + 2, npd)                 # filled past wrap-around
    x = unit_mags(rng, n, npd)
    r0 = rng.uniform(-1, 1, n).astype(npd)
    p = n // 2
    x_nan, x_inf = x.copy(), x.copy()
    x_nan[p], x_inf[p] = np.nan, np.inf
    fl = oracle.scalar_flags(npd, 1.0, 0.0)
    for label, mode, push_mode, exact in QN_FORMS[kind]:
        op, O = make_qn(lo, dev, kind, dtype, n, mem)
        if push_mode:
            op.set_push_mode(push_mode)
        if mode:
            op.set_mode(mode)
        for s, y in prs:
            lo.push(op, T(s, dev), T(y, dev))
            assert op._last_push_accepted == O.push(s, y)
        tol = (TOL_QN_REF if exact else TOL_QN_ALT)[npd]
        base = O.mul(np.empty(n, npd), x, 1.0, 0.0, flags=fl)
        want_nan = O.mul(np.empty(n, npd), x_nan, 1.0, 0.0, flags=fl)
        want_inf = O.mul(np.empty(n, npd), x_inf, 1.0, 0.0, flags=fl)
        want_ab = O.mul(r0.copy(), x_nan, 2.0, -3.0, flags=oracle.scalar_flags(npd, 2.0, -3.0))
        assert np.isnan(want_nan).all() and not np.isfinite(want_inf).any()
        # Inf in x: the sign of the term c_k * a_k[i] (c_k = ±Inf) is the sign of the DERIVED panel entry a_k[i]. The device's
        # panel agrees with the oracle's to the family's tolerance, not to the bit, so where |a_k[i]| <= tol * max|a_k| that
        # sign — and with it ±Inf versus NaN at position i — is not determined by the inputs: there only "not finite" holds.
        # (The inverse operator multiplies the Inf by the stored s, y themselves: no such positions.)
        # Such positions do occur in this data: L-SR1, Float32, n = 2^19, mem 5 holds a_5[50290] = -3.06e-7 next to
        # max|a_5| = 0.918 (the oracle's panel), and the device, whose a_5 differs in the last bits, has -Inf there where
        # the oracle has NaN; 299 of the 5 * 2^19 entries lie below 2e-5 * max|a_k|. They cannot be generated away: a_k is
        # derived from the pairs by the recursion, not chosen.
        amb = np.zeros(n, bool)
        if kind != "inv":
            mx = np.abs(O.a).max(axis=1, keepdims=True)
            amb = ((np.abs(O.a) <= tol * mx) & (mx > 0)).any(axis=0)
        assert amb.mean() <= 0.01
        for sched, small, persist in schedules:
            what = f"{kind} {label} {sched} n={n} mem={mem} {npd.__name__}"
            with ctx.tuned(qn_fused_small=small, qn_persist=persist):
                def run(xv, a=1.0, b=0.0):
                    res = T(r0.copy(), dev)
                    if b == 0:
                        res.fill_(float("nan"))
                    lo.mul(res, op, T(xv, dev), a, b)
                    return res.cpu().numpy()
                check_against_oracle(run(x), base, tol=tol, what=what + " clean")
                check_against_oracle(run(x_nan), want_nan, tol=tol, what=what + " NaN in x")
                check_against_oracle(run(x_nan, 2.0, -3.0), want_ab, tol=tol, what=what + " NaN in x, beta != 0")
                got = run(x_inf)
                if exact:
                    check_against_oracle(got[~amb], want_inf[~amb], tol=tol, what=what + " Inf in x")
                    assert not np.isfinite(got[amb]).any(), what + " Inf in x: a finite element"
                else:
                    assert not np.isfinite(got).any(), what + " Inf in x: a finite element"
                if scaled and n <= 1 << 16:
                    for sc in (UP(npd), DOWN(npd)):
                        xs = reduction_operand((x * sc).astype(npd), npd, scaled=True)
                        want = (base.astype(np.float64) * float(sc)).astype(npd)   # the apply is linear in x
                        check_against_oracle(run(xs), want, tol=tol, what=what + f" x * {sc:g}")
    ctx.sync()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["inv", "fwd", "lsr1"])
@pytest.mark.parametrize("n,mem", [(7, 1), (7, 5), (4099, 1), (4099, 5), (4099, 12), (1 << 16, 5), (1 << 16, 12)])
def test_quasi_newton_apply_nonfinite_x(lo, dev, dtype, kind, n, mem):
    """NaN in x: all NaN in every form. One Inf in x: the reference-ordered forms (inverse `reforder`, push mode `reforder`)
    give the oracle's class map; the two-pass (Gram) inverse apply and the `gram` / `compact` push modes evaluate other
    algebra — their coefficients are ±Inf or NaN and the panels hold no exact zero, so every element is ±Inf or NaN, but
    WHICH of the two may differ from the recursion's: for them the assertion is "no element is finite". x scaled by
    1e120 / 1e-120 (1e15 / 1e-15): the apply is linear, the result is the scale times the unscaled oracle result within
    the family's tolerance. Single-launch and four-launch schedules."""
    if kind == "lsr1" and n <= mem:
        pytest.skip("SR1 with more pairs than dimensions is rounding noise in the reference too (test_gpu_qn.py)")
    _qn_apply_cases(lo, dev, kind, dtype, n, mem, QN_SCHEDULES)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["inv", "fwd", "lsr1"])
def test_quasi_newton_persistent_apply_nonfinite_x(lo, dev, dtype, kind):
    """The persistent form (n = 2^19, mem 5, `qn_persist_min_bytes` = 0): NaN and Inf in x as above."""
    ctx = lo.get_ctx(dev)
    with ctx.tuned(qn_persist_min_bytes=0):
        _qn_apply_cases(lo, dev, kind, dtype, 1 << 19, 5, QN_SCHEDULES[:1], scaled=False)


# =========================================================================== 5. push! with non-finite pairs
PUSH_TUNES = [(fused, posted) for fused in (1, 0) for posted in (1, 0)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["inv", "fwd"])
def test_lbfgs_push_nan_and_inf_pairs(lo, dev, dtype, kind):
    """push!(op, s, y) with a NaN in y is ACCEPTED (`NaN <= eps` is false, src/lbfgs.jl:281): applies (and diag! /
    solve_shifted_system! of the forward operator) have the oracle's class map afterwards, reset! + clean pushes reproduce
    a fresh operator bit for bit; a pair with an Inf follows the oracle's decision (accepted: non-finite wherever the oracle
    is; rejected: nothing changes). Fused and copy schedules, posted and
    read-back scalars, an aligned and a misaligned pair."""
    npd = NP[dtype]
    ctx = lo.get_ctx(dev)
    n, mem = 4099, 5
    rng = np.random.default_rng(12)
    prs = qn_pairs(rng, n, 3, npd)
    x = rng.uniform(-1, 1, n).astype(npd)
    fl = oracle.scalar_flags(npd, 1.0, 0.0)
    for fused, posted in PUSH_TUNES:
        with ctx.tuned(push_fused=fused, push_posted=posted):
            fresh, _ = make_qn(lo, dev, kind, dtype, n, mem)       # (same schedule: the two schedules sum their dots in other orders)
            for s, y in prs:
                lo.push(fresh, T(s, dev), T(y, dev))
            fresh_out = (fresh * T(x, dev)).clone()
            for off in (0, 1):
                for bad in ("nan_y", "inf_y", "inf_s_neg"):
                    what = str((kind, npd.__name__, fused, posted, off, bad))
                    op, O = make_qn(lo, dev, kind, dtype, n, mem)
                    for s, y in prs:
                        lo.push(op, T(s, dev), T(y, dev))
                        O.push(s, y)
                    s, y = (a.copy() for a in qn_pairs(rng, n, 1, npd)[0])
                    if bad == "nan_y":
                        y[n - 3] = np.nan
                    elif bad == "inf_y":
                        s[17], y[17] = abs(s[17]) + npd(0.1), np.inf            # y's = +Inf
                    else:
                        s[17], y[17] = -abs(s[17]) - npd(0.1), np.inf           # y's = -Inf <= eps: rejected by the reference
                    lo.push(op, put(s, dev, off), put(y, dev, off))
                    acc = O.push(s, y)
                    assert op._last_push_accepted == acc, what
                    assert op.data.insert == O.insert, what
                    got = (op * T(x, dev)).cpu().numpy()
                    want = O.mul(np.empty(n, npd), x, 1.0, 0.0, flags=fl)
                    if bad == "nan_y":
                        assert acc and np.isnan(want).all()
                    exact = bad == "nan_y" or not acc      # an accepted Inf pair: the default push modes evaluate other algebra
                    if exact:
                        check_against_oracle(got, want, tol=TOL_QN_ALT[npd], what=what + " apply")
                    else:
                        assert not np.isfinite(got[~np.isfinite(want)]).any(), what + " apply: finite where the oracle is not"
                    if kind == "fwd":
                        dg, dw = lo.diag(op).cpu().numpy(), O.diag()
                        if exact:
                            check_against_oracle(dg, dw, tol=TOL_QN_ALT[npd], what=what + " diag!")
                        else:
                            assert not np.isfinite(dg[~np.isfinite(dw)]).any(), what + " diag!: finite where the oracle is not"
                        if bad == "nan_y":
                            xs = lo.solve_shifted_system(torch.zeros(n, dtype=dtype, device=dev), op, T(x, dev), 0.5).cpu().numpy()
                            ws = O.solve_shifted(np.zeros(n, npd), x, npd(0.5))
                            assert not np.isfinite(ws).any()
                            check_against_oracle(xs, ws, tol=TOL_QN_ALT[npd], what=what + " solve_shifted_system!")
                    lo.reset(op)
                    for s, y in prs:
                        lo.push(op, T(s, dev), T(y, dev))
                    assert torch.equal(op * T(x, dev), fresh_out), what + ": reset! + clean pushes == fresh operator"
    ctx.sync()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_damped_lbfgs_push_nan_pair_takes_the_oracles_branch(lo, dev, dtype):
    """Damped push!(op, s, y[, Bs]) (forward) and push!(op, s, y, α, g[, Bs]) (inverse) with a NaN in y: neither Powell
    comparison is true with NaN, the pair is stored undamped (src/lbfgs.jl:300-320, 336-355); accept flag, insert and the
    class map of the next apply equal the oracle's."""
    npd = NP[dtype]
    ctx = lo.get_ctx(dev)
    n, mem = 4099, 5
    rng = np.random.default_rng(13)
    prs = qn_pairs(rng, n, 2, npd)
    x = rng.uniform(-1, 1, n).astype(npd)
    g = rng.uniform(-1, 1, n).astype(npd)
    fl = oracle.scalar_flags(npd, 1.0, 0.0)
    for fused, posted in PUSH_TUNES:
        with ctx.tuned(push_fused=fused, push_posted=posted):
            for off in (0, 1):
                for kind, with_bs in (("fwd", False), ("fwd", True), ("inv", False), ("inv", True)):
                    what = str((kind, with_bs, npd.__name__, fused, posted, off))
                    op, O = make_qn(lo, dev, kind, dtype, n, mem, damped=True)
                    s, y = (a.copy() for a in qn_pairs(rng, n, 1, npd)[0])
                    y[2048] = np.nan
                    yo = y.copy()
                    for s0, y0 in prs:
                        if kind == "fwd":
                            lo.push(op, T(s0, dev), T(y0, dev))
                            O.push(s0.copy(), y0.copy())
                        else:
                            lo.push(op, T(s0, dev), T(y0.copy(), dev), 0.5, T(g, dev))
                            O.push(s0.copy(), y0.copy(), alpha=npd(0.5), g=g)
                    sd, yd = put(s, dev, off), put(y, dev, off)
                    if kind == "fwd":
                        lo.push(op, sd, yd, *([put(np.zeros(n, npd), dev, off)] if with_bs else []))
                        acc = O.push(s, yo)
                    else:
                        lo.push(op, sd, yd, 0.5, T(g, dev), *([put(np.zeros(n, npd), dev, off)] if with_bs else []))
                        acc = O.push(s, yo, alpha=npd(0.5), g=g)
                    assert op._last_push_accepted == acc and op.data.insert == O.insert, what
                    want = O.mul(np.empty(n, npd), x, 1.0, 0.0, flags=fl)
                    assert np.isnan(want).all()
                    check_against_oracle((op * T(x, dev)).cpu().numpy(), want, tol=TOL_QN_ALT[npd], what=what)
    ctx.sync()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("push_mode", ["gram", "reforder"])
def test_lsr1_push_rejects_nonfinite_pairs_and_leaves_the_operator_untouched(lo, dev, dtype, push_mode):
    """L-SR1 push! with a NaN pair or an Inf in y is REJECTED (`abs(NaN) >= ...` is false, src/lsr1.jl:131,145), as in
    the oracle; the operator's next apply, diag! and scalars are bit-identical to those taken before the push (the fused
    push! writes scratch before it decides)."""
    npd = NP[dtype]
    ctx = lo.get_ctx(dev)
    n, mem = 4099, 5
    rng = np.random.default_rng(14)
    x = T(rng.uniform(-1, 1, n).astype(npd), dev)
    for fused, posted in PUSH_TUNES:
        with ctx.tuned(push_fused=fused, push_posted=posted):
            op, O = make_qn(lo, dev, "lsr1", dtype, n, mem)
            op.set_push_mode(push_mode)
            for s, y in qn_pairs(rng, n, mem + 2, npd):
                lo.push(op, T(s, dev), T(y, dev))
                assert op._last_push_accepted == O.push(s, y)
            before = ((op * x).clone(), lo.diag(op).clone(), op.data._scalars())
            for off in (0, 1):
                for bad in ("nan_y", "nan_s", "inf_y"):
                    what = str((npd.__name__, push_mode, fused, posted, off, bad))
                    s, y = (a.copy() for a in qn_pairs(rng, n, 1, npd)[0])
                    if bad == "nan_y":
                        y[n - 2] = np.nan
                    elif bad == "nan_s":
                        s[3] = np.nan
                    else:
                        y[1000] = np.inf
                    lo.push(op, put(s, dev, off), put(y, dev, off))
                    acc = O.push(s, y)
                    assert not acc, "the oracle rejects this pair"
                    assert op._last_push_accepted == acc, what
                    after = ((op * x), lo.diag(op), op.data._scalars())
                    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1]), what
                    assert after[2][0] == before[2][0] and np.array_equal(after[2][1], before[2][1]) \
                        and np.array_equal(after[2][2], before[2][2]), what
    ctx.sync()


# =========================================================================== 6. dense and structured reductions
HERM_SHAPES = [(64, 0, 1), (257, 0, 1), (512, 0, 1), (512, 0, 0), (512, 1, 1), (257, 1, 1)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n,pad,single", HERM_SHAPES)
def test_hermitian_nonfinite(lo, dev, dtype, n, pad, single):
    """mulHermitian! (src/linalg.jl:97-103): NaN in v (all NaN), one +Inf in v (±Inf in every row, no NaN: the elements
    on and above the diagonal never meet v, so there is no 0 * Inf), NaN in d (one NaN), Inf in the strict lower triangle
    (exactly two Inf, no NaN), v scaled by 1e120 (1e15) — single-launch form (n = 512), two-launch form (`herm_single` = 0,
    and the ragged sizes) and the masked form of an A with an odd leading dimension (pad = 1); NaN on and above the
    diagonal of A stays in place in every case. v holds no zero and A's strict lower triangle neither."""
    npd = NP[dtype]
    ctx = lo.get_ctx(dev)
    rng = np.random.default_rng(n + pad)
    A = unit_mags(rng, (n, n), npd)
    A[np.triu_indices(n)] = np.nan
    d = rng.standard_normal(n).astype(npd)
    v = unit_mags(rng, n, npd)
    r0 = rng.standard_normal(n).astype(npd)

    def dev_matrix(M):
        big = torch.zeros(n, n + pad, dtype=dtype, device=dev)
        big[:, :n] = T(np.ascontiguousarray(M.T), dev)
        return big[:, :n].t()

    with ctx.tuned(herm_single=single):
        for case in ("nan_v", "inf_v", "nan_d", "inf_L", "big_v"):
            Ac, dc, vc = A.copy(), d.copy(), v.copy()
            i, j = n - 2, n // 3
            if case == "nan_v":
                vc[n // 2] = np.nan
            elif case == "inf_v":
                vc[n // 2] = np.inf
            elif case == "nan_d":
                dc[n - 1] = np.nan
            elif case == "inf_L":
                Ac[i, j] = np.inf
            else:
                vc = reduction_operand((vc * UP(npd)).astype(npd), npd, scaled=True)
            H = lo.opHermitian(T(dc, dev), dev_matrix(Ac))
            for a, b in ((1.0, 0.0), (3.0, -4.0)):
                res = T(r0.copy(), dev)
                if b == 0:
                    res.fill_(float("nan"))
                lo.mul(res, H, T(vc, dev), a, b)
                want = oracle.hermitian_mul(r0.copy(), dc, np.tril(Ac, -1), vc, a, b, flags=oracle.scalar_flags(npd, a, b))
                if case == "inf_L" and n > 1:
                    assert np.isinf(want).sum() == 2 and not np.isnan(want).any()
                if case == "nan_v" and n > 1:
                    assert np.isnan(want).all()
                if case == "inf_v":
                    assert np.isinf(want).all()
                check_against_oracle(res.cpu().numpy(), want, tol=TOL_HERM[npd], what=str((n, pad, single, case, a, b)))
    ctx.sync()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("m,n", [(10, 6), (300, 257), (64, 2000), (2048, 1024)])
def test_dense_gemv_nonfinite(lo, dev, dtype, m, n):
    """Dense M*v and M'*u (src/constructors.jl:19-29), the row-band kernel at its smallest admitted shape (2048 x 1024)
    included: a NaN in the vector (all NaN), one Inf in the vector (±Inf by the sign of the column, M has no zero), one
    NaN and one Inf in M (one row / one column), the vector scaled by 1e120 / 1e-120."""
    npd = NP[dtype]
    rng = np.random.default_rng(m * 7 + n)
    M = unit_mags(rng, (m, n), npd)
    for trans in (False, True):
        nin, nout = (m, n) if trans else (n, m)
        x = unit_mags(rng, nin, npd)
        r0 = rng.standard_normal(nout).astype(npd)
        for case in ("nan_x", "inf_x", "nan_M", "inf_M", "big_x", "small_x"):
            Mc, xc = M.copy(), x.copy()
            if case == "nan_x":
                xc[nin // 2] = np.nan
            elif case == "inf_x":
                xc[nin - 1] = np.inf
            elif case == "nan_M":
                Mc[m // 2, n - 1] = np.nan
            elif case == "inf_M":
                Mc[m - 1, n // 2] = -np.inf
            elif case == "big_x":
                xc = reduction_operand((xc * UP(npd)).astype(npd), npd, scaled=True)
            else:
                xc = reduction_operand((xc * DOWN(npd)).astype(npd), npd, scaled=True)
            op = lo.LinearOperatorFromMatrix(TM(Mc, dev))
            op = op.T if trans else op
            for a, b in ((1.0, 0.0), (3.0, -4.0)):
                res = T(r0.copy(), dev)
                if b == 0:
                    res.fill_(float("nan"))
                lo.mul(res, op, T(xc, dev), a, b)
                want = oracle.gemv(r0.copy(), Mc, xc, a, b, trans=trans, flags=oracle.scalar_flags(npd, a, b))
                tol = (TOL_GEMV_BAND if m >= 2048 else TOL_GEMV)[npd]
                check_against_oracle(res.cpu().numpy(), want, tol=tol, what=str((m, n, trans, case, a, b)))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_blockdiagonal_nonfinite_stays_in_its_block(lo, dev, dtype):
    """BlockDiagonalOperator of a dense block, a diagonal and a dense block with boundaries off every tile grid (37, 101,
    263 rows): a NaN / an Inf in the part of v that belongs to one block reaches that block's rows only — the other
    blocks' results are bit-identical to the clean apply — and the whole result has the class map of the per-block
    oracle."""
    npd = NP[dtype]
    rng = np.random.default_rng(44)
    sizes = (37, 101, 263)
    Ms = [(rng.uniform(0.5, 1.5, (k, k)) * rng.choice([-1.0, 1.0], (k, k))).astype(npd) for k in sizes]
    dmid = rng.uniform(0.5, 1.5, sizes[1]).astype(npd)
    BD = lo.BlockDiagonalOperator(lo.LinearOperatorFromMatrix(TM(Ms[0], dev)), lo.opDiagonal(T(dmid, dev)),
                                  lo.LinearOperatorFromMatrix(TM(Ms[2], dev)))
    ntot = sum(sizes)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    v = rng.uniform(0.5, 1.5, ntot).astype(npd)
    clean = (BD * T(v, dev)).cpu().numpy()

    def want_of(vc):
        parts = [oracle.gemv(np.empty(sizes[0], npd), Ms[0], vc[:starts[1]].copy(), 1.0, 0.0, flags=oracle.scalar_flags(npd, 1.0, 0.0)),
                 oracle.diag_mul(np.empty(sizes[1], npd), dmid, vc[starts[1]:starts[2]].copy(), 1.0, 0.0, flags=oracle.scalar_flags(npd, 1.0, 0.0)),
                 oracle.gemv(np.empty(sizes[2], npd), Ms[2], vc[starts[2]:].copy(), 1.0, 0.0, flags=oracle.scalar_flags(npd, 1.0, 0.0))]
        return np.concatenate(parts)

    for blk in range(3):
        for val in (np.nan, np.inf):
            for pos in (starts[blk], starts[blk + 1] - 1):             # first and last element of the block's slice
                vc = v.copy()
                vc[pos] = val
                got = (BD * T(vc, dev)).cpu().numpy()
                check_against_oracle(got, want_of(vc), tol=TOL_GEMV[npd], what=str((blk, val, pos)))
                for other in range(3):
                    if other != blk:
                        sl = slice(starts[other], starts[other + 1])
                        assert np.array_equal(got[sl].view(np.uint8), clean[sl].view(np.uint8)), (blk, other, val, pos)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("layout", ["csc", "csr"])
def test_sparse_nonfinite(lo, dev, dtype, layout):
    """A*x and A'*u of a SparseMatrixCSC, handed over as CSC and as the CSR storage of the same matrix (aliased as the CSC
    of the transpose, N and T swapped): a NaN / Inf in the vector reaches only the rows with a stored entry in that
    column (A*x) or the columns that store that row (A'*u); a stored explicit 0.0 opposite an Inf gives NaN; one column
    and one row are longer than a chunk (3000 and 2594 stored entries; a chunk is 2048)."""
    npd = NP[dtype]
    rng = np.random.default_rng(9)
    m, n = 3500, 2600
    cols = []
    for j in range(n):
        k = 3000 if j == 5 else 1 + (j % 6)
        cols.append(np.sort(rng.choice(m, k, replace=False)))
    cols[6] = np.union1d(cols[6], [11])
    for j in range(7, n):                                             # row 11 holds 2594 entries: longer than a chunk (2048)
        cols[j] = np.union1d(cols[j], [11])
    colptr = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int64)
    rowval = np.concatenate(cols).astype(np.int64)
    nz = (rng.uniform(0.5, 1.5, rowval.size) * rng.choice([-1.0, 1.0], rowval.size)).astype(npd)
    zero_col = 3
    nz[colptr[zero_col]] = 0.0                                        # an explicit stored zero in column 3
    zero_row = int(rowval[colptr[zero_col]])
    Mdev = lo.sparse_csc(colptr, rowval, nz, m, n, index_base=0, device=dev)
    if layout == "csr":
        Mdev = Mdev.to_sparse_csr()
        assert Mdev.values().numel() == nz.size, "the explicit stored zero must survive the layout change"
    Sp = lo.LinearOperatorFromMatrix(Mdev)
    colidx = np.repeat(np.arange(n), np.diff(colptr))

    def scale_of(xc, trans):
        """(|A| |x|).max() over the finite part of x — the scale of test_gpu_sparse.py's bound."""
        xa = np.where(np.isfinite(xc), np.abs(xc.astype(np.float64)), 0.0)
        out = np.zeros(n if trans else m)
        if trans:
            np.add.at(out, colidx, np.abs(nz.astype(np.float64)) * xa[rowval])
        else:
            np.add.at(out, rowval, np.abs(nz.astype(np.float64)) * xa[colidx])
        return out.max()
    for trans in (False, True):
        nin, nout = (m, n) if trans else (n, m)
        x = rng.uniform(0.5, 1.5, nin).astype(npd)
        r0 = rng.standard_normal(nout).astype(npd)
        op = lo.transpose(Sp) if trans else Sp
        for case, pos, val in (("nan", 5 if not trans else 11, np.nan), ("inf", 9 if not trans else 11, np.inf),
                               ("inf_zero", zero_col if not trans else zero_row, np.inf), ("nan_short", nin - 1, np.nan)):
            xc = x.copy()
            xc[pos] = val
            for a, b in ((1.0, 0.0), (2.0, -3.0)):
                res = T(r0.copy(), dev)
                if b == 0:
                    res.fill_(float("nan"))
                lo.mul(res, op, T(xc, dev), a, b)
                want = oracle.csc_mul(r0.copy(), colptr + 1, rowval + 1, nz, m, n, xc, a, b, trans=trans, flags=oracle.scalar_flags(npd, a, b))
                if case == "inf_zero":
                    assert np.isnan(want[zero_row if not trans else zero_col])
                assert np.isfinite(want).any(), "the poison must not reach every row"
                check_against_oracle(res.cpu().numpy(), want, atol=TOL_SPARSE[npd] * (abs(a) * scale_of(xc, trans) + abs(b)),
                                     what=str((trans, case, a, b)))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("shapes", [((64, 64), (64, 64)), ((70, 34), (66, 130)), ((33, 65), (129, 31))])
def test_kron_real_nonfinite(lo, dev, dtype, shapes):
    """kron(A, B) * x = vec(B X A') (src/kron.jl:14-22) as one launch, as two launches with the DMA kernel and in the
    fallback: one Inf in x (the oracle's map of ±Inf and NaN), one NaN in A, x scaled by 1e120 (1e15). Factors hold no
    zero."""
    npd = NP[dtype]
    (ma, na), (mb, nb) = shapes
    rng = np.random.default_rng(ma + 10 * na + 100 * mb)
    A, B, x = unit_mags(rng, (ma, na), npd), unit_mags(rng, (mb, nb), npd), unit_mags(rng, na * nb, npd)
    r0 = rng.standard_normal(ma * mb).astype(npd)
    for case in ("inf_x", "nan_A", "big_x"):
        Ac, xc = A.copy(), x.copy()
        if case == "inf_x":
            xc[(na * nb) // 2 + 3] = np.inf
        elif case == "nan_A":
            Ac[ma // 2, na - 1] = np.nan
        else:
            xc = reduction_operand((xc * UP(npd)).astype(npd), npd, scaled=True)
        K = lo.kron(TM(Ac, dev), TM(B, dev))
        for a, b in ((1.0, 0.0), (2.0, -3.0)):
            res = T(r0.copy(), dev)
            if b == 0:
                res.fill_(float("nan"))
            lo.mul(res, K, T(xc, dev), a, b)
            want = oracle.kron_mul(r0.copy(), Ac, B, xc, a, b, flags=oracle.scalar_flags(npd, a, b))
            check_against_oracle(res.cpu().numpy(), want, tol=TOL_KRON[npd], what=str((shapes, case, a, b)))
    lo.get_ctx(dev).sync()


@pytest.mark.parametrize("form", ["4gemm", "gauss"])
@pytest.mark.parametrize("shapes", [((64, 64), (64, 64)), ((70, 34), (66, 130)), ((33, 65), (129, 31))])
def test_kron_complex_nonfinite(lo, dev, form, shapes):
    """kron of two ComplexF64 factors in both `complex_form`s: one Inf in Re(x), one NaN in Re(A), x scaled by 1e120.

    4-GEMM form (re = Ar*Xr - Ai*Xi, im = Ar*Xi + Ai*Xr, each a real GEMM): the oracle's exact class map in every case — the
    one Inf of a reduction stays the one Inf of the corresponding real GEMM, and the difference / sum of the two GEMMs is the
    difference / sum the oracle forms term by term.

    Gauss form (three real products P1 = (Ar + Ai)*Xr, P2 = Ar*(Xi - Xr), P3 = Ai*(Xr + Xi), re = P1 - P3, im = P1 + P2):
      * NaN in A: a NaN operand makes every one of the three products that reads it NaN, and the oracle's NaN positions
        are exactly the outputs that read it — the EXACT class map is asserted, finite positions to the family's bound;
      * x scaled by 1e120: everything stays finite — asserted to the family's bound;
      * Inf in x: P1, P2 and P3 are all ±Inf wherever the oracle's terms are, and re / im are differences of them: where
        the oracle has +Inf the Gauss form may have NaN (Inf - Inf) and the reverse. Every position of the result is
        non-finite in the oracle (dense factors without a zero); the assertion is "no position is finite".
    Finite positions: max abs <= 1e-12 * ||K||_1 * max|x| (test_gpu_kron.py::test_complex_form_switch_and_what_each_form_
    guarantees, the reference's criterion of test/test_kron.jl:35)."""
    (ma, na), (mb, nb) = shapes
    npd = np.complex128
    rng = np.random.default_rng(ma + 10 * na + 100 * mb + 7)
    cm = lambda shape: (unit_mags(rng, shape, np.float64) + 1j * unit_mags(rng, shape, np.float64)).astype(npd)
    A, B, x = cm((ma, na)), cm((mb, nb)), cm(na * nb)
    r0 = (rng.standard_normal(ma * mb) + 1j * rng.standard_normal(ma * mb)).astype(npd)
    K1 = np.abs(A).sum(axis=0).max() * np.abs(B).sum(axis=0).max()            # ||kron(A, B)||_1
    for case in ("inf_x", "nan_A", "big_x"):
        Ac, xc = A.copy(), x.copy()
        if case == "inf_x":
            xc[(na * nb) // 2 + 3] = complex(np.inf, xc[(na * nb) // 2 + 3].imag)
        elif case == "nan_A":
            Ac[ma // 2, na - 1] = complex(np.nan, Ac[ma // 2, na - 1].imag)
        else:
            xc = reduction_operand((xc * UP(np.float64)).astype(npd), np.float64, scaled=True)
        K = lo.kron(TM(Ac, dev), TM(B, dev), complex_form=form)
        assert K.complex_form == form
        xmax = np.abs(_real_view(xc)[np.isfinite(_real_view(xc))]).max()
        for a, b in ((1.0, 0.0), (2.0, -3.0)):
            res = T(r0.copy(), dev)
            if b == 0:
                res.fill_(complex(float("nan"), float("nan")))
            lo.mul(res, K, T(xc, dev), a, b)
            got = res.cpu().numpy()
            want = oracle.kron_mul(r0.copy(), Ac, B, xc, a, b, flags=oracle.scalar_flags(npd, a, b))
            what = str((form, shapes, case, a, b))
            atol = 1e-12 * (abs(a) * K1 * xmax + abs(b) * np.abs(r0).max())
            if case == "inf_x":
                assert not np.isfinite(_real_view(want)).any()
            if form == "gauss" and case == "inf_x":
                assert not np.isfinite(_real_view(got)).any(), what + ": a finite position"
            else:
                check_against_oracle(got, want, atol=atol, what=what)
    lo.get_ctx(dev).sync()


def _colmajor(X, pad, dtype, dev):
    """n x k column-major device matrix with leading dimension n + pad."""
    big = torch.zeros(X.shape[1], X.shape[0] + pad, dtype=dtype, device=dev)
    big[:, :X.shape[0]] = T(np.ascontiguousarray(X.T), dev)
    return big[:, :X.shape[0]].t()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("family", ["gemv", "gemv_t", "hermitian", "hermitian_single_off", "csc", "csc_t"])
def test_block_apply_poison_stays_in_its_column(lo, dev, dtype, family):
    """`mul!(res::Matrix, op, V::Matrix, α, β)` through mxlo_gemv_block, mxlo_hermitian_mul_block and mxlo_csc_mul_block:
    a NaN (and, second pass, an Inf) in column j of V leaves every other result column bit-identical to the clean run, and
    column j has the class map of the single-vector oracle. k = 5 columns (chunks of 4 + 1 for opHermitian), padded leading
    dimensions, β = 0 on NaN and β != 0. For opHermitian the poisoned element sits inside a diagonal-block tile."""
    npd = NP[dtype]
    ctx = lo.get_ctx(dev)
    rng = np.random.default_rng(61)
    k, j = 5, 3
    if family.startswith("gemv"):
        m, n = 300, 257
        M = unit_mags(rng, (m, n), npd)
        op = lo.LinearOperatorFromMatrix(TM(M, dev))
        trans = family == "gemv_t"
        op = op.T if trans else op
        nin, nout = (m, n) if trans else (n, m)
        single = lambda r, x, a, b: oracle.gemv(r, M, x, a, b, trans=trans, flags=oracle.scalar_flags(npd, a, b))
        tol, atol_of = TOL_GEMV[npd], None
    elif family.startswith("hermitian"):
        n = 512
        A = unit_mags(rng, (n, n), npd)
        A[np.triu_indices(n)] = np.nan
        d = rng.standard_normal(n).astype(npd)
        op = lo.opHermitian(T(d, dev), TM(A, dev))
        nin = nout = n
        single = lambda r, x, a, b: oracle.hermitian_mul(r, d, np.tril(A, -1), x, a, b, flags=oracle.scalar_flags(npd, a, b))
        tol, atol_of = TOL_HERM[npd], None
    else:
        m, n = 900, 700
        dense = unit_mags(rng, (m, n), npd) * (rng.random((m, n)) < 0.02)
        dense[:, 9] = unit_mags(rng, m, npd)
        dense[5, :] = unit_mags(rng, n, npd)
        cols = [np.flatnonzero(dense[:, c]) for c in range(n)]
        colptr = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int64)
        rowval = np.concatenate(cols).astype(np.int64)
        nz = np.concatenate([dense[c_, i_] for i_, c_ in enumerate(cols)]).astype(npd)
        op = lo.LinearOperatorFromMatrix(lo.sparse_csc(colptr, rowval, nz, m, n, index_base=0, device=dev))
        trans = family == "csc_t"
        op = lo.transpose(op) if trans else op
        nin, nout = (m, n) if trans else (n, m)
        single = lambda r, x, a, b: oracle.csc_mul(r, colptr + 1, rowval + 1, nz, m, n, x, a, b, trans=trans, flags=oracle.scalar_flags(npd, a, b))
        absD = np.abs(dense.astype(np.float64))
        atol_of = lambda x, a, b: TOL_SPARSE[npd] * (abs(a) * float(((absD.T if trans else absD) @ np.where(np.isfinite(x), np.abs(x.astype(np.float64)), 0.0)).max()) + abs(b))
        tol = None
    V = unit_mags(rng, (nin, k), npd)
    R0 = rng.standard_normal((nout, k)).astype(npd)
    pos = nin // 2 + 1
    with ctx.tuned(herm_single=0 if family == "hermitian_single_off" else 1):
        for a, b in ((1.0, 0.0), (2.0, -3.0)):
            def run(Vh):
                R = _colmajor(np.full_like(R0, np.nan) if b == 0 else R0, 3, dtype, dev)
                lo.mul(R, op, _colmajor(Vh, 1, dtype, dev), a, b)
                return R.cpu().numpy()
            clean = run(V)
            for c in range(k):
                check_against_oracle(clean[:, c].copy(), single(R0[:, c].copy(), V[:, c].copy(), a, b), tol=tol,
                                     atol=atol_of and atol_of(V[:, c], a, b), what=str((family, "clean", c, a, b)))
            for val in (np.nan, np.inf):
                Vp = V.copy()
                Vp[pos, j] = val
                got = run(Vp)
                for c in range(k):
                    if c != j:
                        assert np.array_equal(got[:, c].copy().view(np.uint8), clean[:, c].copy().view(np.uint8)), (family, val, c, a, b)
                want = single(R0[:, j].copy(), Vp[:, j].copy(), a, b)
                assert not np.isfinite(want).all()
                check_against_oracle(got[:, j].copy(), want, tol=tol, atol=atol_of and atol_of(Vp[:, j], a, b),
                                     what=str((family, val, "poisoned column", a, b)))
    ctx.sync()


# =========================================================================== 7. a composite pass over finished results
def test_composite_tree_with_one_nan(lo, dev):
    """Sum, product, adjoint, vcat and hcat of the leaves above, one NaN in v, against the same tree evaluated with the
    oracle's leaf functions in the reference's evaluation order (sum: `mul!(res, op1, v, α, β); mul!(res, op2, v, α, 1)`,
    src/operations.jl:187-197; product: the inner operator into a temporary, then the outer one; hcat: the blocks one
    after the other with β = 1 from the second on; vcat: block by block; the adjoint of a vcat is the hcat of the
    adjoints, src/cat.jl):
        S = D + M,   P = S * H',   K = [P; D],   W = [D M]
    K*v: H'v is all NaN, so the first n rows are NaN, and the D block is NaN at the one position only. W*[v1; v2] with the
    NaN in v1: one NaN. K'*w with the NaN in the part of w that meets D: one NaN. Finite positions 1e-10 (test_gpu_fuzz.py)."""
    npd = np.float64
    rng = np.random.default_rng(70)
    n, p = 257, 100
    d, M = unit_mags(rng, n, npd), unit_mags(rng, (n, n), npd)
    h = rng.standard_normal(n)
    h /= np.linalg.norm(h)
    D, Mo, H = lo.opDiagonal(T(d, dev)), lo.LinearOperatorFromMatrix(TM(M, dev)), lo.opHouseholder(T(h, dev))
    S = D + Mo
    P = S * H.H
    K = lo.vcat(P, D)
    W = lo.hcat(D, Mo)
    z = lambda k: np.empty(k, npd)

    def S_mul(x, trans=False):                       # (D + M) x  |  (D + M')x
        r = oracle.diag_mul(z(n), d, x, 1.0, 0.0)
        return oracle.gemv(r, M, x, 1.0, 1.0, trans=trans)

    v = unit_mags(rng, n, npd)
    v[p] = np.nan
    want = np.concatenate([S_mul(oracle.householder_mul(z(n), h, v, 1.0, 0.0)), oracle.diag_mul(z(n), d, v, 1.0, 0.0)])
    assert np.isnan(want[:n]).all() and np.isnan(want[n:]).sum() == 1
    check_against_oracle((K * T(v, dev)).cpu().numpy(), want, tol=1e-10, what="K * v")
    # 5-arg form on the same tree
    r0 = rng.standard_normal(2 * n)
    res = T(r0.copy(), dev)
    lo.mul(res, K, T(v, dev), 2.0, -3.0)
    check_against_oracle(res.cpu().numpy(), 2.0 * want - 3.0 * r0, tol=1e-10, what="mul!(res, K, v, 2, -3)")
    # hcat
    v2 = unit_mags(rng, 2 * n, npd)
    v2[p] = np.nan
    wantW = oracle.gemv(oracle.diag_mul(z(n), d, v2[:n].copy(), 1.0, 0.0), M, v2[n:].copy(), 1.0, 1.0)
    assert np.isnan(wantW).sum() == 1
    check_against_oracle((W * T(v2, dev)).cpu().numpy(), wantW, tol=1e-10, what="W * [v1; v2]")
    # adjoint of the vcat: K' w = P' w1 + D w2, P' = H (D + M')
    w = unit_mags(rng, 2 * n, npd)
    w[n + p] = np.nan
    wantK = oracle.householder_mul(z(n), h, S_mul(w[:n].copy(), trans=True), 1.0, 0.0)
    wantK = oracle.diag_mul(wantK, d, w[n:].copy(), 1.0, 1.0)
    assert np.isnan(wantK).sum() == 1
    check_against_oracle((K.H * T(w, dev)).cpu().numpy(), wantK, tol=1e-10, what="K' * w")
    lo.get_ctx(dev).sync()
