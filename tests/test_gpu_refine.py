"""`refine=r` of opCholesky, opLDL and opLU on the device: r steps of iterative refinement per apply, x += F \\ (v - op(M) x),
with the residual and x in Float64 and one rounding to the element type (csrc/linalg.hip, residual_kernel and the xacc
fields of the sweeps). The matrices, step counts and bounds live in refine_cases.py; test_refine_host.py runs a NumPy model
of the scheme on the same cases and shows that the bounds are attainable and that the hard inputs are hard.

Bounds, all derived, none measured on the device.
1. Hard LDL' (small pivots inside every block of 64, unpivoted factorisation): eta = |K x - v|_2 / (|K|_2 |x|_2) <= n eps(T),
   the bound of the factorisation tests WITHOUT their growth factor: not needing it is the point of refinement. Nothing
   is asserted about refine = 0 on the device. (Model: plain solve 12 .. 9700 n eps in Float64, refined <= 0.06 n eps.)
2. Float32 forward error at cond_2 = 1e4: |x - x*|_inf / |x*|_inf <= eps32 against numpy's Float64 solve of the rounded
   matrix: the converged Float64 iterate is accurate to about cond eps64, its rounding costs at most eps32 / 2, the factor
   2 is the margin. (Model: plain solve 190 .. 1500 eps32, refined <= 0.4 eps32.)
3. Well-conditioned Float64 matrices of the factorisation tests, refine = 1: eta_inf <= n eps, their bound and measure.
8. The residual kernels alone: |r - r_np|_i <= (n + 2) eps64 (|A| |x| + |v|)_i, the standard bound of an n-term dot product
   plus the subtraction."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import refine_cases as rc

gpu = pytest.mark.gpu
NB, KB = rc.NB, 8
NP = {torch.float64: np.float64, torch.float32: np.float32}
TD = {np.float64: torch.float64, np.float32: torch.float32}
NAMES = ("malloc", "free", "h2d", "d2h", "d2d", "d2h_bytes", "stream_sync", "device_sync", "event_sync", "memset_async",
         "launch", "blocking_copy")
NAN = float("nan")


def snap(lo):
    a = (C.c_int64 * 12)()
    lo._lib.call("mxlo_debug_counters", a)
    return dict(zip(NAMES, list(a)))


def dev_matrix(A, dtype, dev, ld=None, rowmajor=False):
    """A on the device: column-major in a leading dimension ld >= n with NaN in the padding, or row-major"""
    t = torch.from_numpy(np.array(A, order="C")).to(dtype).to(dev)
    if rowmajor:
        return t.contiguous()
    ld = ld or max(A.shape[0], 1)
    out = torch.full((ld * A.shape[1],), NAN, dtype=dtype, device=dev).as_strided(A.shape, (1, ld))
    out.copy_(t)
    return out


def dev_vec(v, dtype, dev):
    return torch.from_numpy(np.array(v)).to(dtype).to(dev)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def solve_on_device(lo, dev, make, A, v, dtype, refine, trans=False, rowmajor=False):
    n = A.shape[0]
    op = make(dev_matrix(A, dtype, dev, ld=rc.LD.get(n), rowmajor=rowmajor), refine=refine)
    res = torch.full((n,), NAN, dtype=dtype, device=dev)
    lo.mul(res, lo.transpose(op) if trans else op, dev_vec(v, dtype, dev))
    x = host(res)
    assert np.isfinite(x).all()
    return x


# ------------------------------------------------------------------------------------------------ 1. hard LDL'
@gpu
@pytest.mark.parametrize("rowmajor", [False, True], ids=["colmajor", "rowmajor"])
@pytest.mark.parametrize("n", rc.SIZES + [rc.BIG])
def test_refined_ldl_is_backward_stable_without_the_growth_factor(lo, dev, n, rowmajor):
    for npd, steps in rc.LDL_CASES:
        if n == rc.BIG and (npd is not np.float64 or rowmajor):
            continue
        K, v = rc.hard_ldl(n, npd)
        eps = float(np.finfo(npd).eps)
        eta = rc.eta2(K, solve_on_device(lo, dev, lo.opLDL, K, v, TD[npd], steps, rowmajor=rowmajor), v)
        print(f"hard LDL' n={n} {npd.__name__} refine={steps}: eta = {eta / (n * eps):.3g} n eps")
        assert eta <= n * eps, (n, npd, steps, eta / (n * eps))


# ------------------------------------------------------------------------------------------------ 2. Float32 forward error
@gpu
@pytest.mark.parametrize("rowmajor", [False, True], ids=["colmajor", "rowmajor"])
@pytest.mark.parametrize("n", rc.SIZES)
def test_float32_operators_return_the_rounded_solution(lo, dev, n, rowmajor):
    eps = float(np.finfo(np.float32).eps)
    for kind, make, trans in (("spd", lo.opCholesky, False), ("gen", lo.opLU, False), ("gen", lo.opLU, True)):
        A, v = rc.cond1e4(n, kind)
        x = solve_on_device(lo, dev, make, A, v, torch.float32, rc.F32_STEPS, trans=trans, rowmajor=rowmajor)
        err = rc.forward_error(x, np.linalg.solve(A.T if trans else A, v))
        print(f"cond 1e4 {kind}{'-T' if trans else ''} n={n}: {err / eps:.3g} eps32")
        assert err <= eps, (kind, trans, n, err / eps)


# ------------------------------------------------------------------------------------------------ 3. Float64 unchanged
@gpu
@pytest.mark.parametrize("n", rc.WELL_SIZES)
def test_one_step_keeps_the_accuracy_of_the_well_conditioned_cases(lo, dev, n):
    eps = float(np.finfo(np.float64).eps)
    for base, make, trans in (("chol", lo.opCholesky, False), ("ldl", lo.opLDL, False), ("lu", lo.opLU, False), ("lu", lo.opLU, True),
                              ("simple", lo.opLU, False), ("simple", lo.opLU, True)):
        A, v = rc.well(base, n)
        x = solve_on_device(lo, dev, make, A, v, torch.float64, 1, trans=trans)
        eta = rc.eta_inf(A.T if trans else A, x, v)
        assert eta <= n * eps, (base, trans, n, eta / (n * eps))


# ------------------------------------------------------------------------------------------------ operators for 4 - 9
KINDS = ["chol", "ldl", "lu", "lu-T"]
OPS = {}


def operator(lo, dev, kind, n, dtype, refine, rowmajor=False):
    """(operator or its transpose, the matrix the apply inverts), built once per case. chol and lu get the well-conditioned
    matrices, ldl the hard one."""
    base = kind.split("-")[0]
    key = (base, n, dtype, refine, rowmajor)
    if key not in OPS:
        A = rc.hard_ldl(n, NP[dtype])[0] if base == "ldl" else rc.well(base, n)[0]
        make = {"chol": lo.opCholesky, "ldl": lo.opLDL, "lu": lo.opLU}[base]
        Md = dev_matrix(A, dtype, dev, rowmajor=rowmajor)
        OPS[key] = (make(Md, refine=refine) if refine is not None else make(Md), A, Md)
    op, A, _ = OPS[key]
    return (lo.transpose(op), A.T) if kind.endswith("-T") else (op, A)


def rhs(n, k, seed=0):
    rng = np.random.default_rng(9100 + n + seed)
    return rng.standard_normal((n, k)), rng.standard_normal((n, k))


def singles(lo, w, V, R0, a, b):
    out = []
    for j in range(V.shape[1]):
        r = R0[:, j].clone()
        lo.mul(r, w, V[:, j].clone(), a, b)
        out.append(r)
    return out


# ------------------------------------------------------------------------------------------------ 4. block form
@gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_every_column_of_a_refined_block_apply_is_its_vector_apply_bit_for_bit(lo, dev, kind, dtype):
    n = 2 * NB + 1
    w, _ = operator(lo, dev, kind, n, dtype, 2)
    Vh, Rh = rhs(n, 17)
    for a, b in ((2.0, -0.5), (1.0, 0.0)):
        want = singles(lo, w, dev_matrix(Vh, dtype, dev), dev_matrix(Rh, dtype, dev), a, b)
        for k in (1, 3, 8, 9, 17):
            V = dev_matrix(Vh[:, :k], dtype, dev, ld=n + 3)
            R = dev_matrix(Rh[:, :k], dtype, dev, ld=n + 5)
            if not b:
                R.fill_(NAN)                                # beta == 0: res is not read
            lo.mul(R, w, V, a, b)
            for j in range(k):
                assert torch.equal(R[:, j], want[j]), (kind, dtype, k, j, a, b)
            assert torch.isfinite(R).all()


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_refined_res_may_be_v(lo, dev, kind):
    n, k, dtype = 2 * NB + 1, 9, torch.float64
    w, _ = operator(lo, dev, kind, n, dtype, 2)
    Vh, _ = rhs(n, k)
    for a, b in ((2.0, -0.5), (1.0, 0.0)):
        V = dev_matrix(Vh, dtype, dev, ld=n + 3)
        R = dev_matrix(Vh, dtype, dev, ld=n + 5)
        lo.mul(R, w, V, a, b)
        X = dev_matrix(Vh, dtype, dev, ld=n + 3)
        lo.mul(X, w, X, a, b)
        assert torch.equal(X, R), (a, b)
        x = dev_vec(Vh[:, 0], dtype, dev)
        lo.mul(x, w, x, a, b)                               # and the vector apply
        assert torch.equal(x, R[:, 0])


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_a_nan_column_stays_in_its_column_through_the_refinement(lo, dev, kind):
    n, k, dtype = 2 * NB + 1, 9, torch.float64
    w, _ = operator(lo, dev, kind, n, dtype, 2)
    Vh, Rh = rhs(n, k)
    Vp = Vh.copy()
    Vp[:, 2] = np.nan
    clean = dev_matrix(Rh, dtype, dev, ld=n + 5)
    lo.mul(clean, w, dev_matrix(Vh, dtype, dev, ld=n + 3), 2.0, -0.5)
    R = dev_matrix(Rh, dtype, dev, ld=n + 5)
    lo.mul(R, w, dev_matrix(Vp, dtype, dev, ld=n + 3), 2.0, -0.5)
    for j in range(k):
        if j == 2:
            assert not torch.isfinite(R[:, j]).any()
        else:
            assert torch.isfinite(R[:, j]).all() and torch.equal(R[:, j], clean[:, j]), j


# ------------------------------------------------------------------------------------------------ 5. refine = 0
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_refine_0_is_the_path_without_the_keyword(lo, dev, kind):
    n, k, dtype = 2 * NB + 1, 9, torch.float64
    w0, _ = operator(lo, dev, kind, n, dtype, 0)
    wn, _ = operator(lo, dev, kind, n, dtype, None)
    base0, basen = (OPS[(kind.split("-")[0], n, dtype, r, False)][0] for r in (0, None))
    assert [(t.shape, t.dtype, t.stride()) for t in base0._factor] == [(t.shape, t.dtype, t.stride()) for t in basen._factor]
    Vh, Rh = rhs(n, k)
    launches = []
    for w in (w0, wn):
        outs = []
        for V, R in ((dev_vec(Vh[:, 0], dtype, dev), dev_vec(Rh[:, 0], dtype, dev)), (dev_matrix(Vh, dtype, dev), dev_matrix(Rh, dtype, dev))):
            lo.mul(R.clone(memory_format=torch.preserve_format), w, V, 2.0, -0.5)         # warm-up
            torch.cuda.synchronize()
            a = snap(lo)
            lo.mul(R, w, V, 2.0, -0.5)
            outs.append((R, snap(lo)["launch"] - a["launch"]))
        launches.append(outs)
    for (r0, l0), (rn, ln) in zip(*launches):
        assert torch.equal(r0, rn) and l0 == ln
    nblk = (n + NB - 1) // NB
    assert [l for _, l in launches[0]] == [2 * nblk - 1, 2 * (2 * nblk - 1)]


# ------------------------------------------------------------------------------------------------ 6. contract
@gpu
@pytest.mark.parametrize("k", [1, 9])
@pytest.mark.parametrize("kind", KINDS)
def test_a_refined_apply_is_its_launches_and_nothing_else_and_can_be_captured(lo, dev, kind, k):
    n, r, dtype = 2 * NB + 1, 2, torch.float64
    w, _ = operator(lo, dev, kind, n, dtype, r)
    Vh, Rh = rhs(n, k)
    V = dev_vec(Vh[:, 0], dtype, dev) if k == 1 else dev_matrix(Vh, dtype, dev)
    R0 = dev_vec(Rh[:, 0], dtype, dev) if k == 1 else dev_matrix(Rh, dtype, dev)
    runs = []
    for _ in range(2):                                      # the first is the warm-up
        R = R0.clone(memory_format=torch.preserve_format)
        lo.mul(R, w, V, 2.0, -0.5)
        runs.append(R)
    assert torch.equal(runs[0], runs[1])
    R = R0.clone(memory_format=torch.preserve_format)
    gc.collect()
    torch.cuda.synchronize()
    a = snap(lo)
    lo.mul(R, w, V, 2.0, -0.5)
    b = snap(lo)
    torch.cuda.synchronize()
    d = {key: b[key] - a[key] for key in NAMES}
    nblk = (n + NB - 1) // NB
    assert d["launch"] == -(-k // KB) * ((r + 1) * (2 * nblk - 1) + r * lo.linalg.RESIDUAL_LAUNCHES), d
    assert not {key: x for key, x in d.items() if key != "launch" and x}, d
    assert torch.equal(R, runs[0])
    if k == 1:                                              # replay after v changed in place: the bits of the eager apply
        res = R0.clone()
        g = lo.capture_mul(res, w, V, 2.0, -0.5)
        V.mul_(-1.5)
        want = R0.clone()
        lo.mul(want, w, V, 2.0, -0.5)
        res.copy_(R0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(res, want)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_one_block_is_one_launch_per_solve(lo, dev, kind):
    n, r, dtype = NB, 1, torch.float64
    w, _ = operator(lo, dev, kind, n, dtype, r)
    V, R = dev_vec(rhs(n, 1)[0][:, 0], dtype, dev), torch.zeros(n, dtype=dtype, device=dev)
    lo.mul(R, w, V)
    torch.cuda.synchronize()
    a = snap(lo)
    lo.mul(R, w, V)
    assert snap(lo)["launch"] - a["launch"] == (r + 1) + r * lo.linalg.RESIDUAL_LAUNCHES


# ------------------------------------------------------------------------------------------------ 7. snapshot
@gpu
@pytest.mark.parametrize("rowmajor", [False, True], ids=["colmajor", "rowmajor"])
@pytest.mark.parametrize("kind", KINDS)
def test_the_operator_reads_its_snapshot_not_m(lo, dev, kind, rowmajor):
    n, dtype = 2 * NB + 1, torch.float64
    w, _ = operator(lo, dev, kind, n, dtype, 2, rowmajor)
    Md = OPS[(kind.split("-")[0], n, dtype, 2, rowmajor)][2]
    V, R0 = (dev_vec(x[:, 0], dtype, dev) for x in rhs(n, 1))
    before = R0.clone()
    lo.mul(before, w, V, 2.0, -0.5)
    saved = Md.clone(memory_format=torch.preserve_format)
    Md.fill_(NAN)
    after = R0.clone()
    lo.mul(after, w, V, 2.0, -0.5)
    Md.copy_(saved)
    assert torch.equal(after, before) and torch.isfinite(after).all()


# ------------------------------------------------------------------------------------------------ 8. residual entry points
@gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_the_residual_entry_points_alone(lo, dev, n, dtype):
    h, code = lo.device.get_ctx(dev).handle, lo.device.dtype_code(dtype)
    npd, eps = NP[dtype], float(np.finfo(np.float64).eps)
    rng = np.random.default_rng(9300 + n)
    A = rng.standard_normal((n, n)).astype(npd).astype(np.float64)
    S = np.triu(A) + np.triu(A, 1).T
    Vh = rng.standard_normal((n, KB)).astype(npd).astype(np.float64)
    Xh = rng.standard_normal((n, KB))
    ld, ldv = n + 2, n + 3                                  # rows >= n of A and V hold NaN
    Ad, Vd = dev_matrix(A, dtype, dev, ld=ld), dev_matrix(Vh, dtype, dev, ld=ldv)
    Ud = dev_matrix(np.where(np.triu(np.ones((n, n), dtype=bool), 1), A, np.nan), dtype, dev, ld=ld)   # NaN on and below the diagonal
    dg = dev_vec(np.diag(A), dtype, dev)
    Xd = torch.from_numpy(np.asfortranarray(Xh)).to(dev).t().contiguous().t()       # n x 8 doubles, column stride n
    assert Xd.stride() == (1, n) or n == 1
    calls = {"sym": (S, lambda R, k: lo._lib.call("mxlo_sym_residual", h, code, R.data_ptr(), Ud.data_ptr(), ld, dg.data_ptr(), n,
                                                   Vd.data_ptr(), ldv, Xd.data_ptr(), k)),
             "gen-N": (A, lambda R, k: lo._lib.call("mxlo_gen_residual", h, code, R.data_ptr(), Ad.data_ptr(), ld, n, Vd.data_ptr(), ldv,
                                                     Xd.data_ptr(), k, lo._lib.OP_N)),
             "gen-T": (A.T, lambda R, k: lo._lib.call("mxlo_gen_residual", h, code, R.data_ptr(), Ad.data_ptr(), ld, n, Vd.data_ptr(), ldv,
                                                       Xd.data_ptr(), k, lo._lib.OP_T))}
    for name, (B, call) in calls.items():
        out = {}
        for k in (1, KB):
            runs = []
            for _ in range(2):
                R = torch.full((n * KB,), NAN, dtype=torch.float64, device=dev)
                torch.cuda.synchronize()
                a = snap(lo)["launch"]
                call(R, k)
                assert snap(lo)["launch"] - a == lo.linalg.RESIDUAL_LAUNCHES
                runs.append(R)
            assert torch.equal(runs[0][:n * k], runs[1][:n * k]), (name, k)      # two calls: the same bits
            assert torch.isnan(runs[0][n * k:]).all()                             # columns >= k are not written
            out[k] = host(runs[0][:n * k]).reshape(k, n).T
            assert np.isfinite(out[k]).all(), (name, k)                           # no padding and no masked element was read
            want = Vh[:, :k] - B @ Xh[:, :k]
            bound = (n + 2) * eps * (np.abs(B) @ np.abs(Xh[:, :k]) + np.abs(Vh[:, :k]))
            assert (np.abs(out[k] - want) <= bound).all(), (name, k, float((np.abs(out[k] - want) / bound).max()))
        assert np.array_equal(out[1][:, 0], out[KB][:, 0]), name                  # column 0 of a group: the k = 1 call


# ------------------------------------------------------------------------------------------------ 9. ABI refusals
@gpu
@pytest.mark.parametrize("kind", ["chol", "ldl", "lu"])
def test_overlaps_with_the_snapshot_and_the_work_matrices_are_refused_before_any_launch(lo, dev, kind):
    n, k, dtype = 2 * NB + 1, 2, torch.float64
    op = operator(lo, dev, kind, n, dtype, 2)[0]
    h, code = lo.device.get_ctx(dev).handle, lo.device.dtype_code(dtype)
    p = [t.data_ptr() for t in op._factor]
    work = op._factor[-2]
    assert work.numel() == 2 * n * KB                       # the sweeps' matrix, then x
    if kind == "chol":                                      # (W, dinv, work, dg)
        call = lambda res, V: lo._lib.call("mxlo_chol_mul_refine", h, code, res, n, p[0], n, n, p[1], p[3], p[2], V, n, k, 2, 1.0, 0.0)
        extra = {"the diagonal vector": p[3]}
    elif kind == "ldl":                                     # (W, dinv, d, work, dg)
        call = lambda res, V: lo._lib.call("mxlo_ldl_mul_refine", h, code, res, n, p[0], n, n, p[1], p[2], p[4], p[3], V, n, k, 2, 1.0, 0.0)
        extra = {"the diagonal vector": p[4]}
    else:                                                   # (W, dinv_l, dinv_u, perm, work, A2)
        call = lambda res, V: lo._lib.call("mxlo_lu_mul_refine", h, code, res, n, p[0], n, n, p[1], p[2], p[3], p[5], n, p[4], V, n, k, 2,
                                           lo._lib.OP_N, 1.0, 0.0)
        extra = {"the snapshot": p[5]}
    extra["the snapshot in W"] = p[0] + 8 * n               # the strict upper triangle starts in column 1
    extra["the second work matrix"] = work.data_ptr() + 8 * n * KB
    good = torch.ones(n * k, dtype=dtype, device=dev)
    other = torch.ones(n * k, dtype=dtype, device=dev)
    torch.cuda.synchronize()
    before = snap(lo)
    for what, ptr in extra.items():
        for res, V in ((ptr, good.data_ptr()), (good.data_ptr(), ptr)):
            with pytest.raises(lo.MxloError, match="overlap") as e:
                call(res, V)
            assert e.value.status == lo._lib.EINVAL, what
    with pytest.raises(lo.MxloError, match="steps") as e:   # and a step count the operator would have refused
        lo._lib.call("mxlo_chol_mul_refine", h, code, good.data_ptr(), n, p[0], n, n, p[1], p[0], p[2], other.data_ptr(), n, k, 9, 1.0, 0.0)
    assert e.value.status == lo._lib.EINVAL
    assert snap(lo) == before
    call(good.data_ptr(), other.data_ptr())                 # the same call with clean operands goes through
    torch.cuda.synchronize()
    assert torch.isfinite(good).all()
