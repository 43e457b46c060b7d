"""-m gpu: every kernel form a tuning key of the ctx selects (csrc/tune_keys.def), at the small, ragged, misaligned shapes
where kernels go wrong — one case per (key, row, value) of tests/forms_cases.py.

The defaults switch form by size (nt_min_bytes = 256 MiB, qn_persist_min_bytes = 32 MiB, herm_dp_min_bytes = 96 MiB, ...), so
the rest of the suite runs the large-size forms once or twice at one round shape each, and several forms are reached only
when a key is set. The keys exist so that every form can run at any size; this file uses them for that.

Each case runs its family's RUNNER inside `ctx.tuned(**fixed, key=value)` on the session ctx and asserts
  1. parity with the oracle (or the NumPy dense model the family's own test file uses) for the 3-argument form and for
     (alpha, beta) = (2, -3), at the tolerance that file states — bit-exact where that file is bit-exact. The runner does this;
  2. bit-identity with the default-form result (key at its default, `fixed` applied — itself a checked run of the same runner)
     where the row says `bitwise`; otherwise agreement of the two forms at 1e-12 / 2e-5 (tests/test_gpu_qn.py:871). Outputs a
     runner returns under a name that starts with "=" are order-independent by construction (integer-valued data whose
     partial sums are exact in Float64 in any order): they must have the default form's bits under EVERY key;
  3. engagement where the row gives launch counts: the launches of one warmed apply at the row's probe shape. For the five
     forms that may refuse at run time on a shared card (forms_cases.WAIVABLE) the case prints which form ran and waives
     this assertion only;
  4. after the block, every key reads back its enumerated default.

`mxlo_dot`, `mxlo_dot_c` and the sums of `mxlo_diagqn_push` run on integer-valued data (|a_i|, |b_i| <= 2^10, n <= 2^20): the
device scalar must EQUAL the int64 result, so a grid-changing key cannot hide a dropped or doubled element in a tolerance.
The six sums of mxlo_diagqn_push are not exported; they are pinned through SpectralGradient's d[1] = sum(s y) / sum(s^2)
(EQUAL to the quotient of the int64 sums), through the bits of the updated diagonal of the other three kinds (any sum that
changed with the form would change them) and through the oracle.

fused_timeout_ms stays at its default; no case sets fused_debug_drop, alias_guard = 0 or kron_fuse = 2. Nothing here faults
on purpose. Panel columns of a quasi-Newton operator live in the operator's own aligned storage, so the applies never take the
mixed-phase (scalar, four columns per launch) path of the dots kernels, and mxlo_dot has a single column, which shares its own
phase. That path runs through push! with s and y at different 16-byte phases (forms_cases.PUSHMIX): the decision dots are then
panel_dots over the caller's vectors themselves, on several workgroups at n = 4099 and 300 001."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import forms_cases as fc
import oracle
from test_gpu_opnorm import Basis, cgs2, combine, combine_ref, inputs as krylov_inputs, ldvs, off_phase, orth, storage_rounding
from test_gpu_opnorm import rel as rel_ld
from test_gpu_qn import pairs
from tolerances import QN_F32

pytestmark = pytest.mark.gpu

TT = {"f64": torch.float64, "f32": torch.float32, "c128": torch.complex128}
NPT = {"f64": np.float64, "f32": np.float32, "c128": np.complex128}
AB = (None, (2.0, -3.0))                                  # None: the 3-argument form


# ------------------------------------------------------------------------------------------------ helpers
def launches(lo):
    a = (C.c_int64 * 12)()
    lo._lib.call("mxlo_debug_counters", a)
    return a[10]


def counted(lo, fn):
    """kernel launches of one warmed call of fn"""
    fn()
    l0 = launches(lo)
    fn()
    return launches(lo) - l0


def place(x, off, dev):
    """x on the device, its first element `off` elements after a 16-byte boundary (torch allocations are 256-byte aligned)"""
    per16 = max(16 // x.dtype.itemsize, 1)
    buf = torch.zeros(x.size + 2 * per16, dtype=torch.from_numpy(x[:0]).dtype, device=dev)
    view = buf[off:off + x.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    assert view.data_ptr() % 16 == (off * x.dtype.itemsize) % 16
    return view


def cm(X, pad, dev):
    """column-major device matrix with leading dimension rows + pad"""
    big = torch.zeros(X.shape[1], X.shape[0] + pad, dtype=torch.from_numpy(X[:0]).dtype, device=dev)
    big[:, :X.shape[0]] = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
    return big[:, :X.shape[0]].t()


def rnd(rng, shape, npd):
    if np.dtype(npd).kind == "c":
        return (rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)).astype(npd)
    return rng.uniform(-1, 1, shape).astype(npd)


def rel(a, b):
    a, b = np.asarray(a).astype(np.complex128 if np.iscomplexobj(a) or np.iscomplexobj(b) else np.float64), np.asarray(b)
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (nb if nb else 1.0))


def mul(lo, res, op, v, ab):
    if ab is None:
        lo.mul(res, op, v)
    else:
        lo.mul(res, op, v, *ab)
    return res


def ab_of(ab):
    return (1.0, 0.0) if ab is None else ab


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


_REF = {}


def ref(key, make):
    """the oracle's result for a (family, shape, ...) key, computed once and read-only from then on"""
    if key not in _REF:
        out = make()
        for a in (out if isinstance(out, tuple) else (out,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


class Run:
    """what a runner hands back: named outputs and, at the probe shape, the launches of one apply"""

    def __init__(self, row):
        self.row, self.out, self.es, self.launches = row, {}, {}, None

    def put(self, name, value, es=None):
        """es: bytes of the operator's real element type where the output itself is wider (Float64 scalars of a Float32 operator)"""
        assert name not in self.out, name
        self.out[name] = np.asarray(value).copy()
        self.es[name] = es or np.empty(0, self.out[name].dtype).real.dtype.itemsize

    def probe(self, shape):
        return self.row["engaged"] is not None and shape == self.row["probe"]


# ------------------------------------------------------------------------------------------------ elementwise leaves
def run_stream(lo, dev, ctx, R):
    """opDiagonal, opEye, mxlo_scale and the Householder update on both views: bit-exact against the oracle
    (tests/test_gpu_leaves.py, tests/test_gpu_complex.py, tests/test_gpu_abi_direct.py::test_dot_and_householder_apply)"""
    from linearoperators_jl_amd.device import dtype_code, ptr
    for t, n in R.row["shapes"]:
        npd, dtype = NPT[t], TT[t]
        rng = np.random.default_rng(n + 17 * len(t))
        d, v, r0 = rnd(rng, n, npd), rnd(rng, n, npd), rnd(rng, n, npd)
        for off in (0, 1):
            if t == "c128" and off:                        # one element IS 16 bytes
                continue
            dd, vd = place(d, off, dev), place(v, off, dev)
            D = lo.opDiagonal(dd)
            E = lo.opEye(dtype, n, S=lo.Storage(dtype, dev))
            for ab in AB:
                a, b = ab_of(ab)
                fl = oracle.scalar_flags(npd, a, b)
                res = mul(lo, place(r0, off, dev), D, vd, ab)
                got = host(res)
                assert same(got, ref(("diag", t, n, ab), lambda: oracle.diag_mul(r0.copy(), d, v, a, b, flags=fl))), ("diag", t, n, off, ab)
                R.put(f"diag {t} {n} {off} {ab}", got)
                res = mul(lo, place(r0, off, dev), E, vd, ab)
                got = host(res)
                assert same(got, ref(("eye", t, n, ab), lambda: oracle.eye_mul(r0.copy(), v, a, b, flags=fl | oracle.TAIL_BETA))), ("eye", t, n, off, ab)
                R.put(f"eye {t} {n} {off} {ab}", got)
            res = place(r0, off, dev)
            lo.operators._scale(res, -2.5)
            got = host(res)
            assert same(got, ref(("scale", t, n), lambda: oracle.scale(r0.copy(), -2.5, flags=oracle.scalar_flags(npd, -2.5, 0)))), ("scale", t, n, off)
            R.put(f"scale {t} {n} {off}", got)
            if t == "c128":
                continue
            dot = torch.tensor([0.37], dtype=torch.float64, device=dev)
            for alpha, beta in ((1.0, 0.0), (2.0, 0.0), (2.0, -3.0)):
                res = place(r0, off, dev)
                lo._lib.call("mxlo_householder_apply", ctx.handle, dtype_code(dtype), ptr(res), ptr(dd), ptr(vd), n, alpha, beta,
                             lo._lib.SCALARS_F64 if t == "f32" else 0, ptr(dot))
                got = host(res)
                if beta == 0:                              # the elementwise part given the scalar: res = alpha (v - (2 dot) h), no FMA
                    c = npd(2) * npd(0.37)
                    assert same(got, (alpha * (v - c * d).astype(np.float64)).astype(npd)), ("update", t, n, off, alpha)
                R.put(f"update {t} {n} {off} {alpha} {beta}", got)


def run_restrict(lo, dev, ctx, R):
    """range and index-list restriction / extension on both views: bit copies (tests/test_gpu_leaves.py)"""
    for t, n in R.row["shapes"]:
        npd, dtype = NPT[t], TT[t]
        rng = np.random.default_rng(5 * n + len(t))
        v = rnd(rng, n, npd)
        specs = [("list", rng.integers(1, n + 1, max(1, n // 2))), ("perm", rng.permutation(n)[:max(1, n // 3)] + 1),
                 ("unit", lo.jrange(1, n, 1)), ("back", lo.jrange(n, 1, -2)), ("step", lo.jrange(min(2, n), n, 3))]
        for off in (0, 1):
            if t == "c128" and off:
                continue
            vd = place(v, off, dev)
            for name, spec in specs:
                idx = spec.to_numpy() if isinstance(spec, lo.jrange) else np.asarray(spec, dtype=np.int64)
                P = lo.opRestriction(spec, n, device=dev)
                out = place(np.full(idx.size, 7, npd), off, dev)
                lo.mul(out, P, vd)
                got = host(out)
                assert same(got, v[idx - 1]), ("restrict", name, t, n, off)
                R.put(f"restrict {name} {t} {n} {off}", got)
                if name == "list":                         # duplicates: the extension's order of writes is not part of this test
                    continue
                u = v[:idx.size].copy()
                back = place(np.full(n, 7, npd), off, dev)
                lo.mul(back, P.H, place(u, off, dev))
                want = np.zeros(n, npd)
                want[idx - 1] = u
                got = host(back)
                assert same(got, want), ("extend", name, t, n, off)
                R.put(f"extend {name} {t} {n} {off}", got)


def run_extend(lo, dev, ctx, R):
    """mxlo_scatter_zero_sorted (the kernel behind a sorted opExtension) on 4-, 8- and 16-byte elements: res .= 0; res[I] = u with
    I increasing and its last index = nres, res at both 16-byte phases, sizes at a tile boundary +- 1; the guard words around
    res stay untouched"""
    from linearoperators_jl_amd.device import ptr
    for es, nres in R.row["shapes"]:
        words = es // 4
        rng = np.random.default_rng(nres + es)
        for density in (0.5, 0.002):
            idx = np.flatnonzero(rng.random(nres) < density) + 1
            idx = np.union1d(idx, [nres]).astype(np.int64)
            u = rng.integers(1, 2 ** 31 - 1, (idx.size, words), dtype=np.int64).astype(np.int32)      # never an all-zero element
            want = np.zeros((nres, words), np.int32)
            want[idx - 1] = u
            ud, idx_d = torch.from_numpy(u.reshape(-1)).to(dev), torch.from_numpy(idx).to(dev)
            for off in ((0,) if es == 16 else (0, 1)):
                buf = torch.full(((nres + 4) * words,), -559038737, dtype=torch.int32, device=dev)
                rd = buf[off * words:(off + nres) * words]
                lo._lib.call("mxlo_scatter_zero_sorted", ctx.handle, es, ptr(rd), nres, ptr(ud), ptr(idx_d), None, idx.size)
                got = host(buf).reshape(nres + 4, words)
                assert (got[:off] == -559038737).all() and (got[off + nres:] == -559038737).all(), ("wrote outside res", es, nres, off)
                assert same(got[off:off + nres], want), (es, nres, density, off)
                R.put(f"extend {es} {nres} {density} {off}", got[off:off + nres])


# ------------------------------------------------------------------------------------------------ reductions
def run_dots(lo, dev, ctx, R):
    """mxlo_dot / mxlo_dot_c on integer-valued operands: EQUAL to the int64 result, operands at equal and at mixed phases"""
    from linearoperators_jl_amd.device import dtype_code, ptr
    for t, n in R.row["shapes"]:
        a, b, want = fc.dot_exact(t, n)
        for offa, offb in ((0, 0), (1, 1), (0, 1)):
            if t == "c128" and (offa or offb):
                continue
            out = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
            if t == "c128":
                ad, bd = (place((x[0] + 1j * x[1]).astype(np.complex128), 0, dev) for x in (a, b))
                lo._lib.call("mxlo_dot_c", ctx.handle, dtype_code(TT[t], complex_ok=True), ptr(ad), ptr(bd), n, ptr(out))
                got = host(out)
                assert (got[0], got[1]) == (float(want[0]), float(want[1])), (t, n, got, want)
            else:
                ad, bd = place(a.astype(NPT[t]), offa, dev), place(b.astype(NPT[t]), offb, dev)
                lo._lib.call("mxlo_dot", ctx.handle, dtype_code(TT[t]), ptr(ad), ptr(bd), n, ptr(out))
                got = host(out)[:1]
                assert got[0] == float(want), (t, n, offa, offb, got[0], want)
            R.put(f"={t} {n} {offa} {offb}", got)


def run_house(lo, dev, ctx, R):
    """opHouseholder against the oracle at 1e-12 / 1e-5 (tests/test_gpu_leaves.py), h and v at equal and at mixed phases"""
    for t, n in R.row["shapes"]:
        npd = NPT[t]
        rng = np.random.default_rng(100 + n)
        h = rng.standard_normal(n)
        h = (h / np.linalg.norm(h)).astype(npd)
        v, r0 = rnd(rng, n, npd), rnd(rng, n, npd)
        tol = 1e-12 if t == "f64" else 1e-5
        fl = oracle.SCALARS_F64 if t == "f32" else 0
        for offh, offv in ((0, 0), (1, 1), (0, 1)):
            hd, vd = place(h, offh, dev), place(v, offv, dev)
            H = lo.opHouseholder(hd)
            for ab in AB:
                a, b = ab_of(ab)
                want = ref(("house", t, n, ab), lambda: oracle.householder_mul(r0.copy(), h, v, a, b, flags=fl))
                got = host(mul(lo, place(r0, offv, dev), H, vd, ab))
                e = rel(got, want)
                assert e <= tol, ("householder", t, n, offh, offv, ab, e)
                R.put(f"house {t} {n} {offh} {offv} {ab}", got)
            if R.probe((t, n)) and (offh, offv) == (0, 0):
                res = place(r0, 0, dev)
                R.launches = counted(lo, lambda: lo.mul(res, H, vd, 1.0, 0.0))


def run_krylov(lo, dev, ctx, R):
    """mxlo_krylov_orth / mxlo_krylov_combine against NumPy at the bound tests/test_gpu_opnorm.py derives: 8 x the distance
    between the float64 and the longdouble evaluation of the same inputs"""
    for t, n, k in R.row["shapes"]:
        npd, dtype = NPT[t], TT[t]
        V, w, y = krylov_inputs(n, k, npd)

        def bounds():
            w_ref, c_ref = cgs2(V, w, np.float64)
            w_ld, c_ld = cgs2(V, w, np.longdouble)
            w_mod, c_mod = cgs2(V, w, np.float64, storage_rounding(npd))
            o_ref, nrm_ref = combine_ref(V, y, np.float64)
            o_ld, nrm_ld = combine_ref(V, y, np.longdouble)
            o_mod, nrm_mod = combine_ref(V, y, np.float64, storage_rounding(npd))
            return (w_ref, c_ref, 8 * rel_ld(w_mod, w_ld), 8 * rel_ld(c_mod, c_ld), o_ref, nrm_ref, 8 * rel_ld(o_mod, o_ld), 8 * rel_ld(nrm_mod, nrm_ld))
        w_ref, c_ref, tol_w, tol_c, o_ref, nrm_ref, tol_o, tol_n = ref(("krylov", t, n, k), bounds)
        y_dev = torch.from_numpy(y).to(dev)
        for ldv in ldvs(n, dtype):
            for where in ("column", "off phase"):
                basis = Basis(V, ldv, dtype, dev)
                if where == "column":
                    wt = basis.col(k)
                    wt.copy_(torch.from_numpy(w))
                else:
                    keep, wt = off_phase(w, dev)
                st, coef = orth(lo, dev, basis, wt)
                assert st == 0, lo._lib.lib().mxlo_last_error()
                w_out, c_out = host(wt), host(coef)
                e_w, e_c = rel_ld(w_out.astype(np.float64), w_ref), rel_ld(c_out, c_ref)
                print(f"orth {t} n={n} k={k} ldv={ldv} {where}: w {e_w:.3e} (bound {tol_w:.3e}) coef {e_c:.3e} (bound {tol_c:.3e})")
                assert e_w <= tol_w and e_c <= tol_c, ("orth", t, n, k, ldv, where)
                R.put(f"orth w {t} {n} {k} {ldv} {where}", w_out)
                R.put(f"orth coef {t} {n} {k} {ldv} {where}", c_out)
                basis = Basis(V, ldv, dtype, dev)
                if where == "column":
                    out = basis.col(0)
                else:
                    keep, out = off_phase(np.zeros(n, npd), dev)
                st, coef = combine(lo, dev, basis, y_dev, out)
                assert st == 0, lo._lib.lib().mxlo_last_error()
                o_out, n_out = host(out), host(coef)
                e_o, e_n = rel_ld(o_out, o_ref), rel_ld(n_out[0], nrm_ref)
                print(f"combine {t} n={n} k={k} ldv={ldv} {where}: out {e_o:.3e} (bound {tol_o:.3e}) norm {e_n:.3e} (bound {tol_n:.3e})")
                assert e_o <= tol_o and e_n <= tol_n, ("combine", t, n, k, ldv, where)
                R.put(f"combine out {t} {n} {k} {ldv} {where}", o_out)
                R.put(f"combine norm {t} {n} {k} {ldv} {where}", n_out)


def run_diagqn(lo, dev, ctx, R):
    """mxlo_diagqn_push, all four kinds, on integer-valued s, y, d (exact sums in any order): s, y, d aligned and at three
    different phases; the oracle at 1e-12 / 2e-5 (tests/test_gpu_diagqn.py) and, for SpectralGradient, EQUAL to the quotient
    of the int64 sums"""
    for t, kind, n in R.row["shapes"]:
        npd, dtype = NPT[t], TT[t]
        s, y, d, sums = fc.diagqn_exact(n)
        s, y, d = s.astype(npd), y.astype(npd), d.astype(npd)
        tol = 1e-12 if t == "f64" else 2e-5
        per16 = fc.V[t]
        for phases in ((0, 0, 0), (0, 1 % per16, 2 % per16)):
            sd, yd = place(s, phases[0], dev), place(y, phases[1], dev)
            if kind == "spectral":
                B = lo.SpectralGradient(npd(1.5), n, dtype=dtype, device=dev)
                lo.push(B, sd, yd)
                got = host(B.d)
                rT = (lambda x: float(np.float32(x))) if t == "f32" else float
                assert got[0] == npd(rT(rT(sums[2]) / rT(sums[0]))), (t, n, phases, got[0], sums[2] / sums[0])
            else:
                ctor = {"psb": lo.DiagonalPSB, "andrei": lo.DiagonalAndrei, "bfgs": lo.DiagonalBFGS}[kind]
                dd = place(d, phases[2], dev)
                B = ctor(dd)
                lo.push(B, sd, yd)
                got = host(B.d)
                want = ref(("diagqn", t, kind, n), lambda: oracle.DiagonalQN(kind, d.copy()).push(s, y).d.copy())
                e = rel(got, want)
                assert e <= tol, ("diagqn", t, kind, n, phases, e)
            R.put(f"={t} {kind} {n} {phases}", got)


# ------------------------------------------------------------------------------------------------ quasi-Newton operators
def _qn_make(lo, kind, dtype, n, mem, dev):
    return {"inv": lo.InverseLBFGSOperator, "fwd": lo.LBFGSOperator, "lsr1": lo.LSR1Operator}[kind](dtype, n, mem=mem, scaling=True, device=dev)


def _qn_oracle(kind, npd, n, mem):
    return oracle.LSR1(n, mem=mem, scaling=True, dtype=npd) if kind == "lsr1" else oracle.LBFGS(n, mem=mem, scaling=True, inverse=(kind == "inv"), dtype=npd)


def run_qn(lo, dev, ctx, R):
    """L-BFGS (inverse, forward) and L-SR1 applies against the oracle at 1e-9 / QN_F32 (tests/test_gpu_qn.py): memories partly
    filled and wrapped, 3-argument and (2, -3) forms, an x one element off the 16-byte grid (the four-launch path)"""
    for shape in R.row["shapes"]:
        kind, t, mem, n = shape[0], shape[1], shape[2], shape[-1]
        npush = shape[3] if len(shape) == 5 else mem + 2
        npd, dtype = NPT[t], TT[t]
        tol = 1e-9 if t == "f64" else QN_F32
        fl = oracle.SCALARS_F64 if t == "f32" else 0
        rng = np.random.default_rng(n + 31 * mem)
        x, r0 = rnd(rng, n, npd), rnd(rng, n, npd)
        prs = pairs(rng, n, npush, npd)
        stops = sorted({0, min(mem // 2, npush - 1), npush - 1})

        def wants():
            O, out = _qn_oracle(kind, npd, n, mem), {}
            for k, (s, y) in enumerate(prs):
                O.push(s, y)
                if k in stops:
                    for ab in AB:
                        out[(k, ab)] = O.mul(r0.copy(), x, *ab_of(ab), flags=fl)
            return out
        want = ref(("qn", kind, t, mem, npush, n), wants)
        op = _qn_make(lo, kind, dtype, n, mem, dev)
        xd, xm = place(x, 0, dev), place(x, 1, dev)
        for k, (s, y) in enumerate(prs):
            lo.push(op, place(s, 0, dev), place(y, 0, dev))
            if k not in stops:
                continue
            for ab in AB:
                for name, xv in (("x", xd), ("x+1", xm)):
                    got = host(mul(lo, place(r0, 0, dev), op, xv, ab))
                    e = rel(got, want[(k, ab)])
                    assert e <= tol, ("qn", shape, k, ab, name, e)
                    R.put(f"qn {shape} {k} {ab} {name}", got)
        if R.probe(shape):
            res = place(r0, 0, dev)
            R.launches = counted(lo, lambda: lo.mul(res, op, xd, 2.0, -3.0))


def run_invmode(lo, dev, ctx, R):
    """InverseLBFGSOperator created inside the tuned block (qn.hip:3018 reads lbfgs_inv_mode at creation), wrapped memory,
    against the oracle at 1e-9 / QN_F32 (tests/test_gpu_qn.py: 1e-10 reference order, 1e-9 two-pass)"""
    for t, mem, n in R.row["shapes"]:
        npd, dtype = NPT[t], TT[t]
        tol = 1e-9 if t == "f64" else QN_F32
        fl = oracle.SCALARS_F64 if t == "f32" else 0
        rng = np.random.default_rng(n + 7 * mem)
        x, r0 = rnd(rng, n, npd), rnd(rng, n, npd)
        prs = pairs(rng, n, mem + 3, npd)

        def wants():
            O = _qn_oracle("inv", npd, n, mem)
            for s, y in prs:
                O.push(s, y)
            return {ab: O.mul(r0.copy(), x, *ab_of(ab), flags=fl) for ab in AB}
        want = ref(("invmode", t, mem, n), wants)
        op = _qn_make(lo, "inv", dtype, n, mem, dev)
        for s, y in prs:
            lo.push(op, place(s, 0, dev), place(y, 0, dev))
        for ab in AB:
            got = host(mul(lo, place(r0, 0, dev), op, place(x, 0, dev), ab))
            e = rel(got, want[ab])
            assert e <= tol, ("invmode", t, mem, n, ab, e)
            R.put(f"inv {t} {mem} {n} {ab}", got)


def run_push(lo, dev, ctx, R):
    """push! on all three operators, filled past wrap-around, with a rejected pair: the accept / reject decisions (insert
    pointer) EQUAL the oracle's, mxlo_qn_get_scalars and the next apply against the oracle at 1e-6 / 1e-9 / QN_F32
    (tests/test_gpu_qn.py::test_one_pass_push_matches_two_kernel_schedule_and_oracle)"""
    for shape in R.row["shapes"]:
        kind, t, mem, n = shape[:4]
        phases = shape[4] if len(shape) == 5 else None     # (phase of s, phase of y) for every pair: the mixed-phase decision dots
        npd, dtype = NPT[t], TT[t]
        tol = 1e-9 if t == "f64" else QN_F32
        fl = oracle.SCALARS_F64 if t == "f32" else 0
        rng = np.random.default_rng(mem * 7 + n)
        x, r0 = rnd(rng, n, npd), rnd(rng, n, npd)
        prs = pairs(rng, n, mem + 4, npd)
        prs.insert(3, (prs[0][0], (-prs[0][0]).astype(npd)) if kind != "lsr1" else (prs[0][0], np.zeros(n, npd)))   # rejected

        def wants():
            O, ins, scal = _qn_oracle(kind, npd, n, mem), [], []
            for s, y in prs:
                O.push(s, y)
                ins.append(O.insert)
                scal.append(O.scaling_factor)
            return np.array(ins), np.array(scal), {ab: O.mul(r0.copy(), x, *ab_of(ab), flags=fl) for ab in AB}
        ins_want, scal_want, want = ref(("push", kind, t, mem, n), wants)
        op = _qn_make(lo, kind, dtype, n, mem, dev)
        ins, scal, ys = [], [], []
        for k, (s, y) in enumerate(prs):
            offs = phases or ((1, 1) if k % 5 == 4 else (0, 0))   # else: every fifth pair from views one element off the 16-byte grid
            lo.push(op, place(s, offs[0], dev), place(y, offs[1], dev))
            sc, ys_k, aux_k = op.data._scalars()
            ins.append(int(sc[0]))
            scal.append(sc[1])
            ys.append(np.concatenate([ys_k, aux_k]))
        assert np.array_equal(ins, ins_want), ("accept / reject decisions", kind, t, mem, n, ins, list(ins_want))
        assert np.allclose(scal, scal_want, rtol=1e-6 if t == "f64" else 1e-4, atol=0), ("scaling factor", kind, t, mem, n)
        R.put(f"=insert {kind} {t} {mem} {n} {phases}", np.array(ins))
        R.put(f"scaling {kind} {t} {mem} {n} {phases}", np.array(scal), es=np.dtype(npd).itemsize)
        R.put(f"scalars {kind} {t} {mem} {n} {phases}", np.concatenate(ys), es=np.dtype(npd).itemsize)
        for ab in AB:
            got = host(mul(lo, place(r0, 0, dev), op, place(x, 0, dev), ab))
            e = rel(got, want[ab])
            assert e <= tol, ("apply after the pushes", kind, t, mem, n, ab, e)
            R.put(f"apply {kind} {t} {mem} {n} {phases} {ab}", got)


# ------------------------------------------------------------------------------------------------ dense, sparse, kron
def run_gemv(lo, dev, ctx, R):
    """dense LinearOperator(M): M v, M' u, M V and M' U for k = 4, 8, 9 against the float64 product at 1e-12 / 2e-5 (vectors)
    and 1e-12 / 3e-5 (blocks) (tests/test_gpu_ops.py), even and odd leading dimensions of M, V and res"""
    for t, m, n, pad in R.row["shapes"]:
        npd = NPT[t]
        rng = np.random.default_rng(m * 1000 + n)
        Mh = rnd(rng, (m, n), npd)
        W = Mh.astype(np.float64)
        op = lo.LinearOperatorFromMatrix(cm(Mh, pad, dev))
        v, u, r0, r1 = rnd(rng, n, npd), rnd(rng, m, npd), rnd(rng, m, npd), rnd(rng, n, npd)
        tol = 1e-12 if t == "f64" else 2e-5
        for ab in AB:
            a, b = ab_of(ab)
            for name, o, xin, rin, Wm in (("N", op, v, r0, W), ("T", op.T, u, r1, W.T)):
                got = host(mul(lo, place(rin, 0, dev), o, place(xin, 0, dev), ab))
                e = rel(got, a * (Wm @ xin.astype(np.float64)) + b * rin.astype(np.float64))
                assert e <= tol, ("gemv", name, t, m, n, pad, ab, e)
                R.put(f"gemv {name} {t} {m} {n} {pad} {ab}", got)
        if R.probe((t, m, n, pad)):                        # (launches of M v, launches of M V with 4 columns)
            res, vd = place(r0, 0, dev), place(v, 0, dev)
            Rb, Vb = cm(rnd(rng, (m, 4), npd), pad, dev), cm(rnd(rng, (n, 4), npd), pad, dev)
            R.launches = (counted(lo, lambda: lo.mul(res, op, vd, 2.0, -3.0)), counted(lo, lambda: lo.mul(Rb, op, Vb, 2.0, -3.0)))
        tolb = 1e-12 if t == "f64" else 3e-5
        for k in fc.GEMV_K:
            Vh, Uh, R0, R1 = rnd(rng, (n, k), npd), rnd(rng, (m, k), npd), rnd(rng, (m, k), npd), rnd(rng, (n, k), npd)
            for ab in AB:
                a, b = ab_of(ab)
                for name, o, Xin, Rin, Wm in (("N", op, Vh, R0, W), ("T", op.T, Uh, R1, W.T)):
                    res = cm(Rin, pad, dev)
                    mul(lo, res, o, cm(Xin, pad, dev), ab)
                    got = host(res)
                    e = rel(got, a * (Wm @ Xin.astype(np.float64)) + b * Rin.astype(np.float64))
                    assert e <= tolb, ("block gemv", name, t, m, n, pad, k, ab, e)
                    R.put(f"gemvb {name} {t} {m} {n} {pad} {k} {ab}", got)


def run_cgemv(lo, dev, ctx, R):
    """complex dense LinearOperator(M): N, T and C applies against the oracle at 1e-12 (tests/test_gpu_complex.py)"""
    for t, m, n in R.row["shapes"]:
        npd = NPT[t]
        rng = np.random.default_rng(m * 1000 + n)
        Mh, v, u = rnd(rng, (m, n), npd), rnd(rng, n, npd), rnd(rng, m, npd)
        op = lo.LinearOperatorFromMatrix(cm(Mh, 0, dev))
        for ab in ((complex(1), complex(0)), (2.0, -3.0)):
            fl = oracle.scalar_flags(npd, *ab)
            for o, xin, mode, nr in ((op, v, "N", m), (op.T, u, "T", n), (op.H, u, "C", n)):
                r0 = rnd(np.random.default_rng(nr), nr, npd)
                got = host(mul(lo, place(r0, 0, dev), o, place(xin, 0, dev), ab))
                want = ref(("cgemv", t, m, n, mode, ab), lambda: oracle.gemv(r0.copy() if ab[1] != 0 else np.zeros(nr, npd), Mh, xin, *ab, trans=mode, flags=fl))
                e = rel(got, want)
                assert e <= 1e-12, ("cgemv", t, m, n, mode, ab, e)
                R.put(f"cgemv {t} {m} {n} {mode} {ab}", got)


def run_herm(lo, dev, ctx, R):
    """opHermitian(d, A), real and complex, vector and (real) block of 3 columns against the oracle at 1e-12 / 3e-5
    (tests/test_gpu_ops.py, tests/test_gpu_complex.py); NaN on and above the diagonal of A is never read"""
    for t, n in R.row["shapes"]:
        npd = NPT[t]
        cplx = t == "c128"
        rng = np.random.default_rng(n + len(t))
        A = rnd(rng, (n, n), npd)
        d = rng.standard_normal(n).astype(np.float64 if cplx else npd)
        v, r0 = rnd(rng, n, npd), rnd(rng, n, npd)
        Ad = A.copy()
        Ad[np.triu_indices(n)] = np.nan
        H = lo.opHermitian(torch.from_numpy(d).to(dev), cm(Ad, 0, dev))
        tol = 3e-5 if t == "f32" else 1e-12
        L = np.tril(A, -1)
        vd = place(v, 0, dev)
        for ab in (((complex(1), complex(0)), (2.0, -3.0)) if cplx else AB):
            a, b = ab_of(ab)
            fl = oracle.scalar_flags(npd, a, b) if cplx else (oracle.SCALARS_F64 if t == "f32" else 0)
            want = ref(("herm", t, n, ab), lambda: oracle.hermitian_mul(r0.copy(), d, L, v, a, b, flags=fl))
            got = host(mul(lo, place(r0, 0, dev), H, vd, ab))
            e = rel(got, want)
            assert e <= tol, ("hermitian", t, n, ab, e)
            R.put(f"herm {t} {n} {ab}", got)
        if R.probe((t, n)):
            res = place(r0, 0, dev)
            R.launches = counted(lo, lambda: lo.mul(res, H, vd, 2.0, -3.0))
        if cplx:
            continue
        Vh, R0 = rnd(rng, (n, 3), npd), rnd(rng, (n, 3), npd)
        for ab in AB:
            a, b = ab_of(ab)
            fl = oracle.SCALARS_F64 if t == "f32" else 0
            want = ref(("hermb", t, n, ab), lambda: np.stack([oracle.hermitian_mul(R0[:, j].copy(), d, L, Vh[:, j].copy(), a, b, flags=fl) for j in range(3)], axis=1))
            res = cm(R0, 1, dev)
            mul(lo, res, H, cm(Vh, 1, dev), ab)
            got = host(res)
            e = rel(got, want)
            assert e <= tol, ("hermitian block", t, n, ab, e)
            R.put(f"hermb {t} {n} {ab}", got)


def run_kron(lo, dev, ctx, R):
    """kron(A, B): N and T applies against the oracle / the dense Kronecker product at 10 x (1e-12 / 3e-5)
    (tests/test_gpu_kron.py::test_kron_shapes_and_layouts)"""
    for shape in R.row["shapes"]:
        t, (m, n), (p, q) = shape
        npd = NPT[t]
        rng = np.random.default_rng(m + 7 * n + 49 * p + 343 * q)
        A, B = (rng.standard_normal((m, n)) / 4).astype(npd), (rng.standard_normal((p, q)) / 4).astype(npd)
        x, xt, r0, r1 = rnd(rng, n * q, npd), rnd(rng, m * p, npd), rnd(rng, m * p, npd), rnd(rng, n * q, npd)
        tol = 10 * (1e-12 if t == "f64" else 3e-5)
        Kop = lo.kron(cm(A, 0, dev), cm(B, 0, dev))
        xd = place(x, 0, dev)
        for ab in AB:
            a, b = ab_of(ab)
            fl = oracle.scalar_flags(npd, a, b)
            want = ref(("kron", shape, ab), lambda: oracle.kron_mul(r0.copy(), A, B, x, a, b, flags=fl))
            got = host(mul(lo, place(r0, 0, dev), Kop, xd, ab))
            e = rel(got, want)
            assert e <= tol, ("kron", shape, ab, e)
            R.put(f"kron N {shape} {ab}", got)
            # (A (x) B)' vec(Y) = vec(B' Y A) for the column-major p x m matrix Y
            want = ref(("kronT", shape, ab), lambda: a * (B.astype(np.float64).T @ xt.astype(np.float64).reshape(m, p).T @ A.astype(np.float64)).T.reshape(-1)
                       + b * r1.astype(np.float64))
            got = host(mul(lo, place(r1, 0, dev), Kop.T, place(xt, 0, dev), ab))
            e = rel(got, want)
            assert e <= tol, ("kron T", shape, ab, e)
            R.put(f"kron T {shape} {ab}", got)
        if R.probe(shape):
            res = place(r0, 0, dev)
            R.launches = counted(lo, lambda: lo.mul(res, Kop, xd, 2.0, -3.0))


def _sparse_matrix(t, chunks, long_row):
    """rows of exactly 16 entries, 128 rows = one chunk of 2048 entries; with `long_row` the last row holds 5000 entries:
    three pieces of at most 2048 and the fix-up launch"""
    rng = np.random.default_rng(chunks)
    ncol = 6000
    regular = 128 * (chunks - (3 if long_row else 0))
    rows = [np.sort(rng.choice(ncol, size=16, replace=False)) for _ in range(regular)]
    if long_row:
        rows.append(np.sort(rng.choice(ncol, size=5000, replace=False)))
    indptr = np.concatenate([[0], np.cumsum([r.size for r in rows])])
    A = sp.csr_matrix((rng.uniform(-1, 1, indptr[-1]), np.concatenate(rows), indptr), shape=(len(rows), ncol)).tocsc()
    A.sort_indices()
    return A.astype(NPT[t])


def run_sparse(lo, dev, ctx, R):
    """sparse LinearOperator(M): N and T, vector and a block of 3 columns against the oracle at 1e-13 / 2e-6 x scale
    (tests/test_gpu_sparse.py); the chunk count of the N apply is read back from mxlo_csc_info"""
    from test_gpu_sparse import TOL, dev_csc, scale_of
    for t, chunks, long_row in R.row["shapes"]:
        npd, dtype = NPT[t], TT[t]
        A = ref(("sparse A", t, chunks, long_row), lambda: _sparse_matrix(t, chunks, long_row))
        m, n = A.shape
        op = lo.LinearOperatorFromMatrix(dev_csc(A, dev, dtype))
        info = op._csc.info()
        assert info["chunks_n"] == chunks and info["long_rows"] == int(long_row), info
        rng = np.random.default_rng(chunks + 1)
        for trans in (False, True):
            nin, nout = (m, n) if trans else (n, m)
            o = lo.transpose(op) if trans else op
            Vh, R0 = rnd(rng, (nin, 3), npd), rnd(rng, (nout, 3), npd)
            for ab in AB:
                a, b = ab_of(ab)
                fl = (0x1 | 0x8) if t == "f32" else 0
                want = ref(("sparse", t, chunks, trans, ab), lambda: np.stack([oracle.csc_mul(np.zeros(nout, npd) if b == 0 else R0[:, j].copy(), A.indptr + 1, A.indices + 1, A.data,
                                                                                              m, n, Vh[:, j].copy(), a, b, trans=trans, flags=fl) for j in range(3)], axis=1))
                tols = [TOL[dtype] * (abs(a) * scale_of(A.T if trans else A, Vh[:, j]) + abs(b) + 1e-300) for j in range(3)]
                got = host(mul(lo, place(R0[:, 0].copy(), 0, dev), o, place(Vh[:, 0].copy(), 0, dev), ab))
                assert np.abs(got.astype(np.float64) - want[:, 0].astype(np.float64)).max() <= tols[0], ("sparse", t, chunks, trans, ab)
                R.put(f"sparse {t} {chunks} {trans} {ab}", got)
                res = cm(R0, 1, dev)
                mul(lo, res, o, cm(Vh, 1, dev), ab)
                got = host(res)
                assert (np.abs(got.astype(np.float64) - want.astype(np.float64)).max(axis=0) <= tols).all(), ("sparse block", t, chunks, trans, ab)
                R.put(f"sparse block {t} {chunks} {trans} {ab}", got)


def run_blockdiag(lo, dev, ctx, R):
    """the fused BlockDiagonalOperator of tests/test_gpu_ops.py::test_blockdiag_fused against the dense block matrix at 1e-12 / 2e-5"""
    for t in R.row["shapes"]:
        npd, dtype = NPT[t], TT[t]
        rng = np.random.default_rng(2)
        S = lo.Storage(dtype, dev)
        d1, d2 = rng.standard_normal(5).astype(npd), rng.standard_normal(1031).astype(npd)
        M1, M2 = rng.standard_normal((4, 7)).astype(npd), rng.standard_normal((300, 3)).astype(npd)
        ops = [lo.opDiagonal(place(d1, 0, dev)), cm(M1, 0, dev), lo.opEye(dtype, 3, S=S), lo.LinearOperatorFromMatrix(cm(M2, 0, dev)),
               lo.opZeros(dtype, 2, 5, S=S), lo.opDiagonal(place(d2, 0, dev))]
        dense = [np.diag(d1), M1, np.eye(3), M2, np.zeros((2, 5)), np.diag(d2)]
        nr, nc = sum(a.shape[0] for a in dense), sum(a.shape[1] for a in dense)
        D = np.zeros((nr, nc))
        r = c = 0
        for a in dense:
            D[r:r + a.shape[0], c:c + a.shape[1]] = a
            r += a.shape[0]
            c += a.shape[1]
        BD = lo.BlockDiagonalOperator(*ops)
        assert hasattr(BD, "_keepalive")                   # the single-launch path
        tol = 1e-12 if t == "f64" else 2e-5
        x, xt, r0, r1 = rnd(rng, nc, npd), rnd(rng, nr, npd), rnd(rng, nr, npd), rnd(rng, nc, npd)
        for ab in AB:
            a, b = ab_of(ab)
            for name, o, xin, rin, Dm in (("N", BD, x, r0, D), ("T", BD.T, xt, r1, D.T)):
                got = host(mul(lo, place(rin, 0, dev), o, place(xin, 0, dev), ab))
                e = rel(got, a * (Dm @ xin.astype(np.float64)) + b * rin.astype(np.float64))
                assert e <= tol, ("blockdiag", name, t, ab, e)
                R.put(f"blockdiag {name} {t} {ab}", got)


RUNNERS = {"stream": run_stream, "restrict": run_restrict, "extend": run_extend, "dots": run_dots, "house": run_house, "house2": run_house,
           "krylov": run_krylov, "diagqn": run_diagqn, "qn4": run_qn, "qnf": run_qn, "qnp": run_qn, "invmode": run_invmode, "push": run_push,
           "gemv": run_gemv, "cgemv": run_cgemv, "herm": run_herm, "kron": run_kron, "sparse": run_sparse, "blockdiag": run_blockdiag}


# ------------------------------------------------------------------------------------------------ the cases
_BASE = {}


def _value(ctx, table, key, v):
    return table[key][2] // ctx.info()["num_cu"] if v == fc.HI_PER_CU else v


def _run(lo, dev, ctx, row, settings):
    R = Run(row)
    with ctx.tuned(**settings):
        RUNNERS[row["family"]](lo, dev, ctx, R)
        torch.cuda.synchronize()
    return R


def test_every_family_has_a_runner():
    assert {r["family"] for rows in fc.FORMS.values() for r in rows} <= set(RUNNERS)


@pytest.mark.parametrize("key,ri,value", fc.cases(), ids=[f"{k}-{i}-{v if isinstance(v, int) else 'hi'}" for k, i, v in fc.cases()])
def test_form(lo, dev, key, ri, value):
    ctx = lo.get_ctx(dev)
    table = {k: (d, lo_, hi) for k, d, lo_, hi in lo._lib.tune_keys()}
    defaults = {k: d for k, (d, _, _) in table.items()}
    assert {k: ctx.tune_get(k) for k in table} == defaults, "an earlier test left a key set"
    row = fc.FORMS[key][ri]
    val = _value(ctx, table, key, value)
    if (key, ri) not in _BASE:                              # the default form: the key at its default, the row's other keys fixed
        _BASE[(key, ri)] = _run(lo, dev, ctx, row, dict(row["fixed"], **{key: defaults[key]})).out
    base = _BASE[(key, ri)]
    R = _run(lo, dev, ctx, row, dict(row["fixed"], **{key: val}))                       # assertion 1 happens in the runner
    assert {k: ctx.tune_get(k) for k in table} == defaults, "keys after the block"      # assertion 4
    assert set(R.out) == set(base) and len(base) > 0
    worst = 0.0
    for name, got in R.out.items():                                                     # assertion 2
        if row["bitwise"] or name.startswith("="):
            assert same(got, base[name]), (key, val, name, "differs from the default form",
                                           int(np.flatnonzero(np.ravel(got != base[name]))[0]) if got.shape == base[name].shape else None)
        else:
            e = rel(got, base[name])
            worst = max(worst, e / fc.BETWEEN_FORMS[R.es[name]])
            assert e <= fc.BETWEEN_FORMS[R.es[name]], (key, val, name, e)
    if not row["bitwise"]:
        print(f"{key} = {val} [{row['family']}]: largest distance to the default form {worst:.3g} x its tolerance")
    if row["engaged"] is not None:                                                      # assertion 3
        want = row["engaged"][value]
        assert R.launches is not None, "the runner never reached the probe shape"
        if key in fc.WAIVABLE:
            print(f"{key} = {val} at {row['probe']}: {R.launches} launch(es) per apply, {want} expected -> "
                  f"{'the form ran' if R.launches == want else 'the form REFUSED at run time (waived)'}")
        else:
            assert R.launches == want, (key, val, row["probe"], R.launches, want)
