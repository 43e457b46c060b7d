"""Block right-hand sides of opCholesky, opLDL, opLU and triangular opInverse on the device: mul!(R, op, V, α, β) with V an
n x k matrix runs the chain of launches of ONE vector apply per group of 8 columns (csrc/linalg.hip, sweep_block_kernel).

What is asserted. Column j of a block apply equals the single-vector apply of that column BIT FOR BIT (torch.equal), for
every operator, mode, element type, k and position in a group; padding and neighbouring columns are left alone; res may be
V; a NaN or Inf in one column stays in that column; an apply is ceil(k/8) times the launches of a vector apply and nothing
else; the backward error of every column is inside the bound of the vector tests.

Matrices (those of test_gpu_linalg.py, test_gpu_ldl.py and test_gpu_lu.py, seeded). H = G G' + I, symmetrised, G =
randn(n, n) / sqrt(n) from default_rng(5200 + n): opCholesky(H); opInverse of its Cholesky factor (lower) and of the
transpose (upper). K: H with the sign of every entry flipped whose row and column index are both 2 mod 3, a symmetric
permutation of a quasi-definite matrix: opLDL(K). H with its rows rolled down by NB + 1, so that every panel's pivots come
from below its diagonal block: opLU. simple_matrix (U S V', singular values 1 .. 2): opLU in the accuracy test.

Sizes. n: 1, NB - 1, NB, NB + 1 (one block; exact; ragged), 2 NB + 1 and 3 NB + 1 (2 and 3 panels and the turn-around).
k: 1 (the column loop), 2 and 7 (a partial group), 8 (a full one), 9 (a group and one), 17 (two groups and one).

Backward error bound. eta = |A x - v|_inf / (|A|_inf |x|_inf) <= n eps(T), the bound of test_gpu_lu.py / test_gpu_ldl.py
with the constants dropped; it is derived, not measured. numpy's LAPACK solve in the same precision reaches at most
0.03 n eps on these matrices at n = 193 (checked on the host when this file was written)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
NB = 64
KB = 8
NS = [1, NB - 1, NB, NB + 1, 2 * NB + 1, 3 * NB + 1]
KS = [1, 2, 7, 8, 9, 17]
NS32, KS32 = [1, NB + 1, 3 * NB + 1], [2, 9]
KMAX = max(KS)
NP = {torch.float64: np.float64, torch.float32: np.float32}
NAMES = ("malloc", "free", "h2d", "d2h", "d2d", "d2h_bytes", "stream_sync", "device_sync", "event_sync", "memset_async",
         "launch", "blocking_copy")
# operator kinds: (constructor's matrix, transposed apply)
KINDS = {"chol": ("chol", False), "ldl": ("ldl", False), "lu": ("lu", False), "lu-T": ("lu", True), "lower": ("lower", False),
         "lower-T": ("lower", True), "upper": ("upper", False), "upper-T": ("upper", True)}
KINDS_ACC = dict(KINDS, **{"simple": ("simple", False), "simple-T": ("simple", True)})     # the accuracy test adds test_gpu_lu.py's matrix
AB = [(1.0, 0.0), (2.0, -0.5)]


def simple_matrix(rng, n):
    """test/test_aux.jl:3-17 for a real element type: U S V' with singular values 1 .. 2 (n = 1: the single value 1)"""
    U = np.linalg.qr(rng.random((n, n)))[0]
    V = np.linalg.qr(rng.random((n, n)))[0]
    return U @ np.diag(1 + np.arange(n) / max(n - 1, 1)) @ V.T


@functools.lru_cache(maxsize=None)
def matrix(base, n, npd):
    """The matrix the constructor of `base` gets, in the device's precision as a read-only Float64 array"""
    rng = np.random.default_rng(5200 + n)
    G = rng.standard_normal((n, n)) / np.sqrt(n)
    H = G @ G.T + np.eye(n)
    H = (H + H.T) / 2
    if base == "chol":
        A = H
    elif base == "ldl":
        s = np.arange(n) % 3 == 2
        A = np.where(s[:, None] & s[None, :], -H, H)
    elif base == "lu":
        A = np.roll(H, NB + 1, axis=0)
    elif base == "simple":
        A = simple_matrix(np.random.default_rng(6200 + n), n)
    else:
        L = np.linalg.cholesky(H.astype(npd).astype(np.float64))
        A = L if base == "lower" else np.ascontiguousarray(L.T)
    A = A.astype(npd).astype(np.float64)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def rhs(n, npd, seed=0):
    """(V, R0): n x KMAX right-hand sides and initial results, read-only"""
    rng = np.random.default_rng(7200 + n + seed)
    V = rng.standard_normal((n, KMAX)).astype(npd).astype(np.float64)
    R0 = rng.standard_normal((n, KMAX)).astype(npd).astype(np.float64)
    V.setflags(write=False)
    R0.setflags(write=False)
    return V, R0


def dev_matrix(A, dtype, dev, ld=None, rowmajor=False, fill=float("nan")):
    """A on the device: column-major in a leading dimension ld >= n (the padding holds `fill`), or row-major."""
    n = A.shape[0]
    t = torch.from_numpy(np.array(A, order="C")).to(dtype).to(dev)            # a copy: A is read-only
    if rowmajor:
        return t.contiguous()
    ld = ld or max(n, 1)
    buf = torch.full((ld * A.shape[1],), fill, dtype=dtype, device=dev)
    out = buf.as_strided(A.shape, (1, ld))
    out.copy_(t)
    return out


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


OPS = {}


def operator(lo, dev, kind, n, dtype, rowmajor=False):
    """the operator of `kind` (built once per (matrix, n, dtype, layout)) and the matrix its apply inverts"""
    base, trans = KINDS_ACC[kind]
    A = matrix(base, n, NP[dtype])
    key = (base, n, dtype, rowmajor)
    if key not in OPS:
        Md = dev_matrix(A, dtype, dev, rowmajor=rowmajor)
        make = {"chol": lo.opCholesky, "ldl": lo.opLDL, "lu": lo.opLU, "simple": lo.opLU}.get(base, lo.opInverse)
        OPS[key] = make(Md)
    op = OPS[key]
    return (lo.transpose(op), A.T) if trans else (op, A)


def singles(lo, w, V, R0, a, b):
    """the k single-vector applies of mul!(r, w, v, a, b), as contiguous vectors"""
    out = []
    for j in range(V.shape[1]):
        r = R0[:, j].clone()
        lo.mul(r, w, V[:, j].clone(), a, b)
        out.append(r)
    return out


def snap(lo):
    a = (C.c_int64 * 12)()
    lo._lib.call("mxlo_debug_counters", a)
    return dict(zip(NAMES, list(a)))


def chain(kind, n):
    nblk = (n + NB - 1) // NB
    return nblk if KINDS[kind][0] in ("lower", "upper") else 2 * nblk - 1


# ------------------------------------------------------------------------------------------------ 1. bit for bit
def check_bit_for_bit(lo, dev, kind, n, dtype, ks, rowmajor=False):
    w, _ = operator(lo, dev, kind, n, dtype, rowmajor)
    Vh, Rh = rhs(n, NP[dtype])
    nan = float("nan")
    for a, b in AB:
        Vall = dev_matrix(Vh, dtype, dev)
        Rall = dev_matrix(Rh, dtype, dev) if b else torch.full((n, KMAX), nan, dtype=dtype, device=dev).t().contiguous().t()
        want = singles(lo, w, Vall[:, :max(ks)], Rall, a, b)
        for k in ks:
            V = dev_matrix(Vh[:, :k], dtype, dev, ld=n + 3)
            R = dev_matrix(Rh[:, :k], dtype, dev, ld=n + 5)
            if not b:
                R.fill_(nan)                                # beta == 0: res is not read
            lo.mul(R, w, V, a, b)
            for j in range(k):
                assert torch.equal(R[:, j], want[j]), (kind, n, dtype, k, j, a, b)
            assert torch.isfinite(R).all()


@gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_column_of_a_block_apply_is_its_single_apply_bit_for_bit_f64(lo, dev, kind, n):
    check_bit_for_bit(lo, dev, kind, n, torch.float64, KS)


@gpu
@pytest.mark.parametrize("n", NS32)
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_column_of_a_block_apply_is_its_single_apply_bit_for_bit_f32(lo, dev, kind, n):
    check_bit_for_bit(lo, dev, kind, n, torch.float32, KS32)


@gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_row_major_m_exchanges_the_modes_in_the_block_form_too(lo, dev, kind, dtype):
    check_bit_for_bit(lo, dev, kind, 2 * NB + 1, dtype, [9], rowmajor=True)


# ------------------------------------------------------------------------------------------------ 2. padding
@gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_padding_and_neighbouring_columns_are_untouched(lo, dev, kind):
    """res and V are the columns 1 .. k + 1 of wider tensors with padded leading dimensions: every element outside the
    n x k windows keeps its sentinel (bitwise: the sentinel is a number), V itself too"""
    n, dtype = 2 * NB + 1, torch.float64
    w, _ = operator(lo, dev, kind, n, dtype)
    Vh, Rh = rhs(n, NP[dtype])
    for k in (3, 9):
        ldr, ldv = n + 5, n + 3
        rbuf = torch.full((ldr * (k + 2),), 7.25, dtype=dtype, device=dev)
        vbuf = torch.full((ldv * (k + 2),), -3.5, dtype=dtype, device=dev)
        R = rbuf.as_strided((n, k), (1, ldr), ldr)
        V = vbuf.as_strided((n, k), (1, ldv), ldv)
        R.copy_(torch.from_numpy(Rh[:, :k].copy()).to(dev))
        V.copy_(torch.from_numpy(Vh[:, :k].copy()).to(dev))
        v0 = vbuf.clone()
        lo.mul(R, w, V, 2.0, -0.5)
        assert torch.equal(vbuf, v0)
        inside = torch.zeros(ldr * (k + 2), dtype=torch.bool, device=dev)
        inside.as_strided((n, k), (1, ldr), ldr).fill_(True)
        assert (rbuf[~inside] == 7.25).all()
        assert (rbuf[inside] != 7.25).all() and torch.isfinite(rbuf).all()


# ------------------------------------------------------------------------------------------------ 3. in place, aliasing
@gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_res_may_be_v(lo, dev, kind):
    n, k, dtype = 2 * NB + 1, 9, torch.float64
    w, _ = operator(lo, dev, kind, n, dtype)
    Vh, _ = rhs(n, NP[dtype])
    for a, b in AB:
        V = dev_matrix(Vh[:, :k], dtype, dev, ld=n + 3)
        R = dev_matrix(Vh[:, :k], dtype, dev, ld=n + 5)
        lo.mul(R, w, V, a, b)                               # out of place, res holding a copy of V
        X = dev_matrix(Vh[:, :k], dtype, dev, ld=n + 3)
        lo.mul(X, w, X, a, b)
        assert torch.equal(X, R), (a, b)


def abi_args(lo, dev, kind, n, dtype):
    """(entry point, head arguments before res, arguments between ldr and V, tail after k) of the operator's own storage"""
    base, trans = KINDS[kind]
    op = operator(lo, dev, kind.split("-")[0], n, dtype)[0]
    h = lo.device.get_ctx(dev).handle
    code = lo.device.dtype_code(dtype)
    mode = lo._lib.OP_T if trans else lo._lib.OP_N
    f = op._factor
    p = [t.data_ptr() for t in f]
    if base == "chol":
        return "mxlo_chol_mul_block", (h, code), (p[0], n, n, p[1], p[2]), ()
    if base == "ldl":
        return "mxlo_ldl_mul_block", (h, code), (p[0], n, n, p[1], p[2], p[3]), ()
    if base == "lu":
        return "mxlo_lu_mul_block", (h, code), (p[0], n, n, p[1], p[2], p[3], p[4]), (mode,)
    return "mxlo_trisolve_mul_block", (h, code), (p[0], n, n, 1 if base == "upper" else 0, mode, p[1], p[2]), ()


def abi_call(lo, name, head, mid, tail, res, ldr, V, ldv, k, a=1.0, b=0.0):
    lo._lib.call(name, *head, res, ldr, *mid, V, ldv, k, *tail, a, b)


@gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_partial_overlap_and_another_leading_dimension_are_refused_before_any_launch(lo, dev, kind):
    n, k, dtype = 2 * NB + 1, 9, torch.float64
    name, head, mid, tail = abi_args(lo, dev, kind, n, dtype)
    buf = torch.ones((n + 2) * (k + 2), dtype=dtype, device=dev)
    torch.cuda.synchronize()
    p = buf.data_ptr()
    before = snap(lo)
    for res, ldr in ((p + 8 * n, n),                        # res is V shifted by one column
                     (p, n + 2)):                           # the same pointer, another leading dimension
        with pytest.raises(lo.MxloError, match="overlaps") as e:
            abi_call(lo, name, head, mid, tail, res, ldr, p, n, k)
        assert e.value.status == lo._lib.EINVAL
    abi_call(lo, name, head, mid, tail, p, n, p, n, 0)      # k == 0: MXLO_OK, nothing to do
    after = snap(lo)
    assert after == before, {key: after[key] - before[key] for key in NAMES}
    with pytest.raises(lo.MxloError, match="overlaps"):     # the same through mul!
        lo.mul(buf.as_strided((n, k), (1, n), n), operator(lo, dev, kind, n, dtype)[0], buf.as_strided((n, k), (1, n)), 1.0, 0.0)
    assert snap(lo) == before
    torch.cuda.synchronize()
    assert torch.equal(buf, torch.ones_like(buf))


@gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_call_through_the_abi_equals_mul_and_the_work_matrix_holds_a_full_group(lo, dev, kind):
    """the operator's own storage handed to the entry point by hand: the same bits as mul!; and the work matrix the
    constructor allocated is n x 8 doubles, what a full group writes"""
    n, k, dtype = 2 * NB + 1, 9, torch.float64
    w, _ = operator(lo, dev, kind, n, dtype)
    work = operator(lo, dev, kind.split("-")[0], n, dtype)[0]._factor[-1]
    assert work.dtype is torch.float64 and work.is_contiguous() and work.numel() >= KB * n
    Vh, Rh = rhs(n, NP[dtype])
    V = dev_matrix(Vh[:, :k], dtype, dev, ld=n + 3)
    want = dev_matrix(Rh[:, :k], dtype, dev, ld=n + 5)
    lo.mul(want, w, V, 2.0, -0.5)
    R = dev_matrix(Rh[:, :k], dtype, dev, ld=n + 5)
    name, head, mid, tail = abi_args(lo, dev, kind, n, dtype)
    abi_call(lo, name, head, mid, tail, R.data_ptr(), n + 5, V.data_ptr(), n + 3, k, 2.0, -0.5)
    assert torch.equal(R, want)


# ------------------------------------------------------------------------------------------------ 4. columns do not mix
@gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_nan_and_an_inf_stay_in_their_columns(lo, dev, kind):
    n, k, dtype = 2 * NB + 1, 9, torch.float64
    w, _ = operator(lo, dev, kind, n, dtype)
    Vh, Rh = rhs(n, NP[dtype])
    Vp = Vh[:, :k].copy()
    Vp[NB + 3, 2] = np.nan                                  # one in the first group ...
    Vp[5, 8] = np.inf                                       # ... one in the group of the ninth column
    V = dev_matrix(Vp, dtype, dev, ld=n + 3)
    R0 = dev_matrix(Rh[:, :k], dtype, dev)
    want = singles(lo, w, V, R0, 2.0, -0.5)
    R = dev_matrix(Rh[:, :k], dtype, dev, ld=n + 5)
    lo.mul(R, w, V, 2.0, -0.5)
    for j in range(k):
        if j in (2, 8):
            assert not torch.isfinite(want[j]).all()
            assert torch.equal(torch.isnan(R[:, j]), torch.isnan(want[j])), j
            assert torch.equal(torch.isinf(R[:, j]), torch.isinf(want[j])), j
        else:
            assert torch.isfinite(R[:, j]).all() and torch.equal(R[:, j], want[j]), j


# ------------------------------------------------------------------------------------------------ 5. launch contract
@gpu
@pytest.mark.parametrize("k", [2, 8, 9])
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_block_apply_is_the_launches_of_one_vector_apply_per_group_and_nothing_else(lo, dev, kind, k):
    import gc
    n, dtype = 4 * NB + 3, torch.float64
    w, _ = operator(lo, dev, kind, n, dtype)
    Vh, Rh = rhs(n, NP[dtype])
    V = dev_matrix(Vh[:, :k], dtype, dev)
    R0 = dev_matrix(Rh[:, :k], dtype, dev)
    runs = []
    for _ in range(2):                                      # the first is the warm-up
        R = R0.clone(memory_format=torch.preserve_format)
        lo.mul(R, w, V, 2.0, -0.5)
        runs.append(R)
    assert torch.equal(runs[0], runs[1])
    R = R0.clone(memory_format=torch.preserve_format)
    assert R.stride() == (1, n)
    gc.collect()
    torch.cuda.synchronize()
    a = snap(lo)
    lo.mul(R, w, V, 2.0, -0.5)
    b = snap(lo)
    torch.cuda.synchronize()
    d = {key: b[key] - a[key] for key in NAMES}
    assert d["launch"] == -(-k // KB) * chain(kind, n), d
    assert not {key: x for key, x in d.items() if key != "launch" and x}, d
    assert torch.equal(R, runs[0])


# ------------------------------------------------------------------------------------------------ 6. accuracy
def eta_inf(A, x, v):
    nx = np.abs(x).max()
    return float(np.abs(A @ x - v).max() / (np.abs(A).sum(axis=1).max() * nx)) if nx else float(np.abs(v).max())




@gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", list(KINDS_ACC))
def test_backward_error_of_the_worst_column(lo, dev, kind, dtype):
    n, k = 3 * NB + 1, 9
    w, A = operator(lo, dev, kind, n, dtype)
    Vh, _ = rhs(n, NP[dtype])
    eps = float(torch.finfo(dtype).eps)
    R = torch.full((n, k), float("nan"), dtype=dtype, device=dev).t().contiguous().t()
    lo.mul(R, w, dev_matrix(Vh[:, :k], dtype, dev))
    X = host(R)
    assert np.isfinite(X).all()
    worst = max(eta_inf(A, X[:, j], Vh[:, j]) for j in range(k))
    print(f"eta_inf {kind} n={n} k={k} {dtype}: worst column {worst:.3e} = {worst / (n * eps):.3e} n eps")
    assert worst <= n * eps, (kind, dtype, worst / (n * eps))       # derived (module docstring)


# ------------------------------------------------------------------------------------------------ 7. shapes
@gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_wrongly_shaped_operands_raise_before_any_launch(lo, dev, kind):
    n, k, dtype = NB + 1, 3, torch.float64
    w, _ = operator(lo, dev, kind, n, dtype)
    good = lambda r, c: torch.ones((c, r), dtype=dtype, device=dev).t()
    torch.cuda.synchronize()
    before = snap(lo)
    with pytest.raises(lo.LinearOperatorException, match="shape mismatch"):
        lo.mul(good(n, k), w, good(n + 1, k), 1.0, 0.0)
    with pytest.raises(lo.LinearOperatorException, match="shape mismatch"):
        lo.mul(good(n, k + 1), w, good(n, k), 1.0, 0.0)
    assert snap(lo) == before
