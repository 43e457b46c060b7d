"""-m gpu: the callers on either side of the path driving the operators the way Krylov.jl /
JSOSolvers do — only through `mul!`, `push!`, `reset!`, `solve_shifted_system!`:
  * conjugate gradients (3-arg and 5-arg `mul!`) on an SPD composite  H * D * H'  (test_linop.jl:346-358 shape);
  * an L-BFGS minimisation loop  d = -(H*g); x += t d; push!(H, s, y)  on a convex quadratic;
  * a trust-region-flavoured use of the forward operator with `solve_shifted_system!`.
Also checks that the all-reduce hook aliases the library's device scalars (a doubling hook must double h'v)."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def cg(lo, A, b, tol=1e-12, maxit=500):
    """Textbook CG written against the operator API only (what Krylov.jl's cg does with mul!(y, A, x))."""
    x = torch.zeros_like(b)
    r = b.clone()
    p = r.clone()
    Ap = torch.empty_like(b)
    rs = torch.dot(r, r)
    for it in range(maxit):
        lo.mul(Ap, A, p)                       # 3-arg mul!
        alpha = rs / torch.dot(p, Ap)
        x += alpha * p
        lo.mul(r, A, p, -float(alpha), 1.0)    # r = r - alpha*A*p as ONE 5-arg mul!
        rs_new = torch.dot(r, r)
        if rs_new.sqrt() <= tol * torch.linalg.vector_norm(b):
            return x, it + 1
        p = r + (rs_new / rs) * p
        rs = rs_new
    return x, maxit


def test_cg_on_composite_spd_operator(lo, dev):
    rng = np.random.default_rng(0)
    n = 2000
    h = rng.standard_normal(n); h /= np.linalg.norm(h)
    lam = np.linspace(1.0, 50.0, n)
    H = lo.opHouseholder(T(h, dev))
    A = H * lo.opDiagonal(T(lam, dev)) * H.H + 0.5 * lo.opEye(torch.float64, n, S=lo.Storage(torch.float64, dev))
    Hd = np.eye(n) - 2 * np.outer(h, h)
    Ad = Hd @ np.diag(lam) @ Hd.T + 0.5 * np.eye(n)
    b = rng.standard_normal(n)
    x, its = cg(lo, A, T(b, dev))
    assert its < 200
    assert np.linalg.norm(Ad @ x.cpu().numpy() - b) <= 1e-9 * np.linalg.norm(b)
    assert lo.nprod(A) == 2 * its               # counters are bumped by the caller-facing mul!


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_lbfgs_minimisation_loop(lo, dev, dtype):
    """min ½ xᵀQx − cᵀx with Q = blockdiag(diagonals) + low-rank, exact line search; the inverse operator
    supplies directions, the forward one tracks the Hessian; both converge and stay consistent."""
    rng = np.random.default_rng(1)
    n, mem = 50_000, 8
    npd = np.float64 if dtype == torch.float64 else np.float32
    q = T(rng.uniform(1.0, 20.0, n).astype(npd), dev)
    u = T((rng.standard_normal(n) / np.sqrt(n)).astype(npd), dev)
    c = T(rng.standard_normal(n).astype(npd), dev)
    Q = lo.opDiagonal(q) + 3.0 * lo.LinearOperatorFromMatrix(u.view(n, 1)) * lo.LinearOperatorFromMatrix(u.view(n, 1)).T
    Hk = lo.InverseLBFGSOperator(dtype, n, mem=mem, device=dev)
    Bk = lo.LBFGSOperator(dtype, n, mem=mem, device=dev)
    x = torch.zeros(n, dtype=dtype, device=dev)
    g = -c.clone()                               # gradient Qx - c at x = 0
    d = torch.empty_like(x)
    Qd = torch.empty_like(x)
    g0 = float(torch.linalg.vector_norm(g))
    for it in range(60):
        lo.mul(d, Hk, g, -1.0, 0.0)              # d = -H g   (the JSOSolvers call shape)
        lo.mul(Qd, Q, d)
        t = -float(torch.dot(g, d)) / float(torch.dot(d, Qd))
        s = t * d
        y = t * Qd                                # y = Q s
        x += s
        g += y
        lo.push(Hk, s, y)
        lo.push(Bk, s, y)
        if Bk._last_push_accepted:               # pairs with y's <= eps(T) are rejected (src/lbfgs.jl:281-284)
            s_acc, y_acc = s.clone(), y.clone()
        if float(torch.linalg.vector_norm(g)) <= (1e-10 if dtype == torch.float64 else 1e-4) * g0:
            break
    assert float(torch.linalg.vector_norm(g)) <= (1e-8 if dtype == torch.float64 else 1e-3) * g0, it
    # secant equation on the most recent ACCEPTED pair: B s = y and H y = s
    tol = 1e-8 if dtype == torch.float64 else 1e-3
    s, y = s_acc, y_acc
    assert float(torch.linalg.vector_norm(Bk * s - y) / torch.linalg.vector_norm(y)) <= tol
    assert float(torch.linalg.vector_norm(Hk * y - s) / torch.linalg.vector_norm(s)) <= tol
    # regularised Newton-like step through the forward operator: (B + σI) p = -g
    p = lo.solve_shifted_system(torch.zeros_like(x), Bk, -g, 0.5)
    resid = (Bk * p) + 0.5 * p + g
    assert float(torch.linalg.vector_norm(resid)) <= (1e-8 if dtype == torch.float64 else 1e-2) * max(1e-30, float(torch.linalg.vector_norm(g)) + 1e-12) + (1e-12 if dtype == torch.float64 else 1e-5)
    lo.reset(Hk)
    assert torch.equal(Hk * c, c)                # back to the identity


def test_allreduce_hook_aliases_device_scalars(lo, dev):
    """A hook that DOUBLES the buffer in place must double h'v as seen by the update kernel: proves the
    tensor handed to torch.distributed aliases the library's device memory (no copy)."""
    rng = np.random.default_rng(2)
    n = 4097
    h = rng.standard_normal(n); h /= np.linalg.norm(h)
    v = rng.uniform(-1, 1, n)
    ctx = lo.get_ctx(dev)
    seen = []

    def hook(user, buf, count, stream):
        t = lo.sharded.wrap_doubles(int(buf), int(count), cuda=True)
        seen.append(float(t[0]))
        t.mul_(2.0)
        return 0

    H = lo.opHouseholder(T(h, dev))
    try:
        ctx.set_allreduce(hook)
        got = (H * T(v, dev)).cpu().numpy()
    finally:
        ctx.set_allreduce(None)
    dot = float(h @ v)
    assert abs(seen[0] - dot) <= 1e-12 * max(1.0, abs(dot))
    want = v - 2 * (2 * dot) * h
    assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)
    # a failing hook surfaces as MXLO_EREDUCE, not as an exception crossing the ABI
    try:
        ctx.set_allreduce(lambda *a: 1)
        with pytest.raises(lo.MxloError) as e:
            H * T(v, dev)
        assert e.value.status == lo._lib.EREDUCE
    finally:
        ctx.set_allreduce(None)


def test_hipgraph_replay_of_apply_sequences(lo, dev):
    """mxlo_graph_*: a recorded sequence of applies replays with one launch and reads the CURRENT contents of
    its buffers; results are bit-identical to the eager calls (same kernels, same order)."""
    rng = np.random.default_rng(8)
    n = 70_001
    h = rng.standard_normal(n); h /= np.linalg.norm(h)
    H = lo.opHouseholder(T(h, dev))
    D = lo.opDiagonal(T(rng.uniform(0.5, 2, n), dev))
    B = lo.LBFGSOperator(n, mem=5, device=dev)
    for _ in range(6):
        s = rng.uniform(-1, 1, n)
        lo.push(B, T(s, dev), T(s * rng.uniform(0.5, 2, n), dev))
    op = H * D + B                                       # composite: compose + sum + quasi-Newton apply
    v = T(rng.uniform(-1, 1, n), dev)
    res, ref = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
    g = lo.capture_mul(res, op, v, 2.0, 0.0)
    for trial in range(3):
        v.copy_(T(rng.uniform(-1, 1, n), dev))           # new data in the SAME buffer
        res.fill_(float("nan"))
        g.replay()
        lo.mul(ref, op, v, 2.0, 0.0)
        assert torch.equal(res, ref), trial
    # several calls in one capture, beta != 0 (res is read and written in place at replay)
    x = T(rng.uniform(-1, 1, n), dev)
    acc, acc_ref = torch.zeros_like(x), torch.zeros_like(x)
    lo.mul(acc, B, x, 1.0, 0.0)                           # warm-up outside the capture
    acc.zero_()
    g2 = lo.CapturedSequence(dev)
    with g2:
        lo.mul(acc, B, x, 1.0, 1.0)
        lo.mul(acc, H, x, -0.5, 1.0)
    for _ in range(2):
        g2.replay()
        lo.mul(acc_ref, B, x, 1.0, 1.0)
        lo.mul(acc_ref, H, x, -0.5, 1.0)
    assert torch.equal(acc, acc_ref)
    # push! synchronises: not capturable -> a clean error, and the ctx keeps working afterwards
    y2 = x * 2.0
    with pytest.raises(lo.MxloError):
        with lo.CapturedSequence(dev):
            lo.push(B, x, y2)
    lo.mul(ref, B, x)
    assert torch.isfinite(ref).all()


def test_alternating_streams_share_the_ctx_workspaces_safely(lo, dev):
    """The ctx's reduction workspace is ordered by its stream; mxlo_ctx_set_stream chains old -> new with an event,
    so applies issued alternately from two torch streams (no host sync in between) never overlap on it."""
    rng = np.random.default_rng(31)
    n = 3_000_017
    hs = [rng.standard_normal(n) for _ in range(2)]
    Hs = [lo.opHouseholder(T(h / np.linalg.norm(h), dev)) for h in hs]
    vs = [T(rng.uniform(-1, 1, n), dev) for _ in range(2)]
    want = [(Hs[i] * vs[i]).clone() for i in range(2)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    outs = [[torch.empty(n, dtype=torch.float64, device=dev) for _ in range(6)] for _ in range(2)]
    for rep in range(6):
        for i in range(2):
            with torch.cuda.stream(streams[i]):
                lo.mul(outs[i][rep], Hs[i], vs[i])
    torch.cuda.synchronize()
    for i in range(2):
        for rep in range(6):
            assert torch.equal(outs[i][rep], want[i]), (i, rep)


def test_graph_replay_direct_chain_equals_hipgraph_launch(lo, dev):
    """Short captured chains replay as direct launches of the recorded nodes (mxlo_graph_info[1] == 1); forcing
    hipGraphLaunch (tune graph_direct_max = 0) must give bit-identical results, for a kernel-only chain, a chain with a
    memset node (index extension through the ABI's memset + scatter entry point) and a quasi-Newton apply."""
    import ctypes as C
    from linearoperators_jl_amd.device import get_ctx, ptr
    ctx = lo.get_ctx(dev)
    rng = np.random.default_rng(5)
    n = 50_000
    h = rng.standard_normal(n); h /= np.linalg.norm(h)
    d = rng.standard_normal(n)
    ht, dt_ = torch.from_numpy(h).to(dev), torch.from_numpy(d).to(dev)
    B = lo.LBFGSOperator(n, mem=4, device=dev)
    for _ in range(5):
        s = rng.uniform(-1, 1, n)
        lo.push(B, torch.from_numpy(s).to(dev), torch.from_numpy(s * rng.uniform(0.5, 2, n)).to(dev))
    op = lo.opHouseholder(ht) * lo.opDiagonal(dt_) + B
    v = torch.from_numpy(rng.uniform(-1, 1, n)).to(dev)
    outs = []
    for direct_max in (16, 0):
        with ctx.tuned(graph_direct_max=direct_max):
            res = torch.from_numpy(np.full(n, 0.5)).to(dev)
            g = lo.capture_mul(res, op, v, 2.0, -3.0)
            inf = g.info()
            assert inf["nodes"] >= 3 and inf["direct"] == (direct_max > 0 and inf["nodes"] <= 16), inf
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize()
            outs.append(res.cpu().numpy().copy())
    assert np.array_equal(outs[0], outs[1])
    # memset node: mxlo_scatter_zero = hipMemsetAsync + scatter kernel
    idx = torch.from_numpy(np.sort(rng.choice(n, 1000, replace=False) + 1).astype(np.int64)).to(dev)
    u = torch.from_numpy(rng.standard_normal(1000)).to(dev)
    outs = []
    for direct_max in (16, 0):
        with ctx.tuned(graph_direct_max=direct_max):
            res = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
            with lo.CapturedSequence(dev) as g:
                c = get_ctx(dev)
                lo._lib.call("mxlo_scatter_zero", c.handle, 8, ptr(res), n, ptr(u), ptr(idx), None, 1000)
            assert g.info()["direct"] == (direct_max > 0)
            res.fill_(7.0)
            g.replay()
            torch.cuda.synchronize()
            outs.append(res.cpu().numpy().copy())
    want = np.zeros(n); want[idx.cpu().numpy() - 1] = u.cpu().numpy()
    assert np.array_equal(outs[0], want) and np.array_equal(outs[1], want)


def test_dense_operator_aliases_row_major_and_column_major_matrices(lo, dev):
    """LinearOperator(M) aliases M like the reference closure (src/constructors.jl:19-29): an in-place update of M after
    construction is seen by the next mul!, for torch's default row-major layout (N/T swapped internally, no copy) and
    for column-major storage alike; kron(LinearOperator(M), B) aliases too."""
    rng = np.random.default_rng(3)
    m, n = 37, 53
    for layout in ("row-major", "column-major"):
        Mh = rng.standard_normal((m, n))
        M = torch.from_numpy(Mh).to(dev) if layout == "row-major" else torch.from_numpy(Mh.T.copy()).to(dev).t()
        assert M.shape == (m, n)
        op = lo.LinearOperatorFromMatrix(M)
        x, u = torch.from_numpy(rng.standard_normal(n)).to(dev), torch.from_numpy(rng.standard_normal(m)).to(dev)
        for _ in range(2):
            y = torch.from_numpy(rng.standard_normal(m)).to(dev)
            y0 = y.cpu().numpy().copy()
            lo.mul(y, op, x, 2.0, -3.0)
            want = 2.0 * (M.cpu().numpy() @ x.cpu().numpy()) - 3.0 * y0
            assert np.linalg.norm(y.cpu().numpy() - want) <= 1e-12 * np.linalg.norm(want), layout
            z = op.T * u
            wt = M.cpu().numpy().T @ u.cpu().numpy()
            assert np.linalg.norm(z.cpu().numpy() - wt) <= 1e-12 * np.linalg.norm(wt), layout
            M.mul_(-1.5).add_(0.25)                       # in place: the operator must follow
            lo.touched(M)
        B = torch.from_numpy(rng.standard_normal((4, 5))).to(dev)
        K = lo.kron(op, B)
        xk = torch.from_numpy(rng.standard_normal(n * 5)).to(dev)
        for _ in range(2):
            want = np.kron(M.cpu().numpy(), B.cpu().numpy()) @ xk.cpu().numpy()
            got = (K * xk).cpu().numpy()
            assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want), layout
            M.mul_(0.5)
            lo.touched(M)


@pytest.mark.parametrize("second", [pytest.param(1, marks=pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs 2 visible devices (one process, current device != operator device)")),
                                    pytest.param(0, id="dry-run-on-the-only-device")])
def test_operator_on_second_device_while_first_is_current(lo, second):
    """One process, two GPUs: every entry point binds ctx->device itself (DeviceGuard), so an operator living on cuda:1
    allocates, launches and copies on cuda:1 while the thread's current device stays cuda:0. (`second` = 0: the same
    statements with the operator on cuda:0 — the dry run of this test's body on a one-GPU box, VERDICT r5 #8.)"""
    torch.cuda.set_device(0)
    d1 = torch.device("cuda", second)
    rng = np.random.default_rng(4)
    n, mem = 20_003, 4
    T1 = lambda a: torch.from_numpy(a).to(d1)
    B = lo.LBFGSOperator(torch.float64, n, mem=mem, device=d1)
    O = oracle.LBFGS(n, mem=mem, inverse=False)
    for _ in range(mem + 2):
        s = rng.uniform(-1, 1, n); y = s * rng.uniform(0.5, 2.0, n)
        lo.push(B, T1(s), T1(y)); O.push(s, y)
        assert torch.cuda.current_device() == 0
    x = rng.uniform(-1, 1, n)
    got = (B * T1(x)).cpu().numpy()
    want = O.mul(np.empty(n), x)
    assert np.linalg.norm(got - want) <= 1e-10 * np.linalg.norm(want)
    h = rng.standard_normal(n); h /= np.linalg.norm(h)
    gh = (lo.opHouseholder(T1(h)) * T1(x)).cpu().numpy()
    assert np.linalg.norm(gh - oracle.householder_mul(np.empty(n), h, x, 1.0, 0.0)) <= 1e-12 * np.linalg.norm(x)
    A = T1(rng.standard_normal((300, 300)))
    Hm = lo.opHermitian(T1(rng.standard_normal(300)), A.t().contiguous().t())
    lo.mul(torch.empty(300, dtype=torch.float64, device=d1), Hm, T1(rng.standard_normal(300)), 1.0, 0.0)
    sol = lo.solve_shifted_system(torch.zeros(n, dtype=torch.float64, device=d1), B, T1(x), 0.5)
    assert torch.isfinite(sol).all() and torch.cuda.current_device() == 0


def test_storage_type_kwarg_mirror(lo, dev):
    """1:1 mirror of the reference's ONLY device tests — /root/reference/test/gpu/test_S_kwarg.jl:3-45 and
    test/gpu/amdgpu.jl:4-20 — with the Python mirror's device types: `arrayType(rand(Float32, 32, 32))` is a Float32 torch
    matrix on the GPU, `storage_type` values are `Storage(dtype, device)`. Same assertions in the same order (the Julia
    statement of the same list is julia/runtests_mxlo.jl, checked textually by tests/test_julia_binding.py); on top of
    the reference's type-only checks the BlockDiagonalOperator of three plain matrices is also compared numerically."""
    f32 = torch.float32
    mat = torch.rand(32, 32, dtype=f32, device=dev).t()                    # Julia layout
    vec = torch.rand(32, dtype=f32, device=dev)
    vecT = lo.storage_type(vec)
    vecTother = lo.storage_type(torch.rand(32, dtype=f32, device=dev))
    assert vecT == lo.storage_type(mat) == lo.Storage(f32, dev)
    # constructors.jl
    assert lo.storage_type(lo.LinearOperatorFromMatrix(mat)) == lo.storage_type(mat)                         # default
    assert lo.storage_type(lo.LinearOperatorFromMatrix(mat, S=vecTother)) == vecTother
    assert lo.storage_type(lo.LinearOperatorFromMatrix(mat, symmetric=True, hermitian=True, S=vecT)) == vecT  # Symmetric(mat)
    assert lo.storage_type(lo.LinearOperatorFromMatrix(mat, symmetric=True, hermitian=True, S=vecT)) == vecT  # Hermitian(mat)
    assert lo.storage_type(lo.LinearOperator(f32, 32, 32, True, True, lambda: 0, S=vecT)) == vecT
    # special-operators.jl
    assert lo.storage_type(lo.opEye(f32, 32, S=vecT)) == vecT
    assert lo.storage_type(lo.opEye(f32, 16, 32, S=vecT)) == vecT
    assert lo.storage_type(lo.opEye(f32, 32, 32, S=vecT)) == vecT
    assert lo.storage_type(lo.opOnes(f32, 32, 32, S=vecT)) == vecT
    assert lo.storage_type(lo.opZeros(f32, 32, 32, S=vecT)) == vecT
    assert lo.storage_type(lo.opDiagonal(vec)) == vecT
    assert lo.storage_type(lo.opDiagonal(32, 32, vec)) == vecT
    assert lo.storage_type(lo.opRestriction([1, 2, 3], 32, S=vecT)) == vecT
    assert lo.storage_type(lo.opExtension([1, 2, 3], 32, S=vecT)) == vecT
    assert lo.storage_type(lo.BlockDiagonalOperator(mat, mat)) == vecT                                       # default
    assert lo.storage_type(lo.BlockDiagonalOperator(mat, mat, S=vecTother)) == vecTother
    # test/gpu/amdgpu.jl:4-20
    A, B, C = (torch.rand(k, k, dtype=f32, device=dev).t() for k in (5, 10, 20))
    M = lo.BlockDiagonalOperator(A, B, C)
    v = torch.rand(35, dtype=f32, device=dev)
    y = M * v
    assert isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == f32                                       # y isa ROCArray{Float32}
    dense = torch.block_diag(A, B, C).double().cpu().numpy()
    assert np.linalg.norm(y.cpu().numpy() - dense @ v.double().cpu().numpy()) <= 3e-5 * np.linalg.norm(dense @ v.double().cpu().numpy())
    yt = M.T * v
    assert np.linalg.norm(yt.cpu().numpy() - dense.T @ v.double().cpu().numpy()) <= 3e-5 * np.linalg.norm(dense.T @ v.double().cpu().numpy())
    assert lo.storage_type(A) == lo.storage_type(A.t().conj())                                               # adjoint(A)
    assert lo.storage_type(A) == lo.storage_type(A.t())                                                      # transpose(A)
    assert lo.storage_type(lo.opDiagonal(v)) == lo.storage_type(v)                                           # Diagonal(v)


def test_cg_on_a_sparse_poisson_operator_preconditioned_by_a_fused_block_diagonal(lo, dev):
    """The Krylov.jl call shape on the sparse leaf (round 4): CG on A = 7-point Laplacian of a 24^3 grid + 0.1 I, held as
    a SparseMatrixCSC-style operator (`mxlo_csc_mul`), written against `mul!` only. A is symmetric: `transpose(A)` must
    give the same iterates through the T-mode sweep (the CSC arrays themselves). The solution is checked against scipy's
    direct solve, and the operator-level identity (A + D) x = A x + D x against a sum with a diagonal operator."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    g = 24
    n = g ** 3
    I1 = sp.identity(g, format="csc")
    L1 = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(g, g), format="csc")
    A = (sp.kron(sp.kron(L1, I1), I1) + sp.kron(sp.kron(I1, L1), I1) + sp.kron(sp.kron(I1, I1), L1) + 0.1 * sp.identity(n)).tocsc()
    A.sort_indices()
    Ad = torch.sparse_csc_tensor(torch.from_numpy(A.indptr.astype(np.int64)), torch.from_numpy(A.indices.astype(np.int64)),
                                 torch.from_numpy(A.data), size=A.shape).to(dev)
    op = lo.LinearOperatorFromMatrix(Ad, symmetric=True, hermitian=True)
    rng = np.random.default_rng(3)
    b = rng.standard_normal(n)
    x, its = cg(lo, op, T(b, dev), tol=1e-11, maxit=400)
    want = spla.spsolve(A, b)
    assert its < 400
    assert np.linalg.norm(x.cpu().numpy() - want) <= 1e-8 * np.linalg.norm(want)
    assert lo.nprod(op) == 2 * its
    xt, its_t = cg(lo, lo.transpose(op), T(b, dev), tol=1e-11, maxit=400)       # symmetric flag: transpose(op) IS op (src/adjtrans.jl)
    assert its_t == its and torch.equal(xt, x)
    raw = lo.LinearOperatorFromMatrix(Ad)                                       # without the flag the T-mode sweep runs
    y1, y2 = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    v = T(rng.standard_normal(n), dev)
    lo.mul(y1, raw, v)
    lo.mul(y2, lo.transpose(raw), v)
    assert float((y1 - y2).abs().max()) <= 1e-12 * float(y1.abs().max())
    d = T(rng.uniform(1, 2, n), dev)
    S = op + lo.opDiagonal(d)
    lo.mul(y1, S, v, 2.0, 0.0)
    assert np.abs(y1.cpu().numpy() - 2.0 * (A @ v.cpu().numpy() + d.cpu().numpy() * v.cpu().numpy())).max() <= 1e-11 * float(y1.abs().max())


def test_block_cg_on_an_ophermitian_operator(lo, dev):
    """A block Krylov caller: conjugate gradients on k = 4 right-hand sides at once, every iteration ONE `mul!` of
    `opHermitian(d, A)` on an n x 4 matrix (src/operations.jl:34-36 — the block entry point reads the triangle once for the
    four columns) and columnwise dots / axpys through the elementwise leaves. Against NumPy's direct solve; and the SAME
    iterations driven column by column give the same iterates bit for bit (the block apply is bit-identical per column)."""
    rng = np.random.default_rng(12)
    n, k = 1500, 4
    A = rng.standard_normal((n, n)) / np.sqrt(n)
    L = np.tril(A, -1)
    d = np.abs(rng.standard_normal(n)) + 4.0                 # diagonally dominant: SPD
    Cm = L + L.T + np.diag(d)
    Bh = rng.standard_normal((n, k))
    H = lo.opHermitian(T(d, dev), T(np.ascontiguousarray(A.T), dev).t())   # column-major A

    def cm(X):
        return T(np.ascontiguousarray(X.T), dev).t()         # column-major device matrix

    def block_cg(apply):
        X = cm(np.zeros((n, k)))
        R, P, Q = cm(Bh.copy()), cm(Bh.copy()), cm(np.zeros((n, k)))
        rs = (R * R).sum(0)
        for _ in range(60):
            apply(Q, P)                                       # Q = H P: one block apply (or k single ones)
            alpha = rs / (P * Q).sum(0)
            X += P * alpha
            R -= Q * alpha
            rs_new = (R * R).sum(0)
            P.mul_(rs_new / rs).add_(R)
            rs = rs_new
        return X

    Xb = block_cg(lambda Q, P: lo.mul(Q, H, P))
    want = np.linalg.solve(Cm, Bh)
    assert np.linalg.norm(Xb.cpu().numpy() - want) <= 1e-10 * np.linalg.norm(want)

    def by_columns(Q, P):
        for j in range(k):
            lo.mul(Q[:, j], H, P[:, j])
    Xc = block_cg(by_columns)
    assert torch.equal(Xb, Xc)
