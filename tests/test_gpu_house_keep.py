"""The kept form of the Householder dot launch (csrc/house_keep.h): the dot workgroups keep their last rounds of h and v
in registers and LDS, exchange their partial sums and update that tail themselves; the update launch gets the prefix.
It engages by itself only at HBM sizes, so the tests force it at small n with existing tune keys
(nt_min_bytes = 0, house_inline_n = 0, house_fused_per_cu = 1) and compare with the oracle and, bit for bit, with the
three-launch path (house_fused = 0 under the same keys)."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

NP = {torch.float64: np.float64, torch.float32: np.float32}
TOL = {torch.float64: 1e-12, torch.float32: 1e-5}
KEPT = 14 + 4                     # kHouseKeepKR + kHouseKeepKL
FORCE = dict(nt_min_bytes=0, house_inline_n=0, house_fused_per_cu=1)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) or 1.0))


def launches(lo):
    a = (C.c_int64 * 12)()
    lo._lib.call("mxlo_debug_counters", a)
    return a[10]


def round_elems(ctx, dtype):
    """Elements of one grid-stride round: num_cu workgroups x 1024 vectors of 16 bytes."""
    return ctx.info()["num_cu"] * 1024 * (16 // torch.empty(0, dtype=dtype).element_size())


def sizes(ctx, dtype):
    R = round_elems(ctx, dtype)
    # 2R + 1 lies below the single-launch limit of house_fused_per_cu = 1 (4R elements): raised by two whole rounds
    return {"two_rounds": 4 * R + 1, "plan_shrinks": KEPT * R + 7, "one_streamed_round": (KEPT + 1) * R,
            "largest_remainder": (KEPT + 1) * R + R - 1, "ragged": (KEPT + 3) * R + 12345}


SIZE_NAMES = ("two_rounds", "plan_shrinks", "one_streamed_round", "largest_remainder", "ragged")


def operands(dev, dtype, n, seed):
    """(h, v, r0) as numpy arrays of n + 1 elements: views [off:off + n] give both 16-byte phases."""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(n + 1).astype(NP[dtype])
    h /= np.linalg.norm(h.astype(np.float64))
    v = rng.uniform(-1, 1, n + 1).astype(NP[dtype])
    r0 = rng.uniform(-1, 1, n + 1).astype(NP[dtype])
    return h, v, r0


def apply(lo, ctx, res, H, v, alpha, beta, fused):
    """One mul! under the forcing keys; returns the number of launches it took."""
    with ctx.tuned(house_fused=fused, **FORCE):
        l0 = launches(lo)
        lo.mul(res, H, v, alpha, beta)
        return launches(lo) - l0


@pytest.mark.parametrize("size", SIZE_NAMES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_kept_form_matches_oracle_and_three_launch_path(lo, dev, dtype, size):
    ctx = lo.get_ctx(dev)
    n = sizes(ctx, dtype)[size]
    assert n > 4 * round_elems(ctx, dtype), "must exceed the single-launch limit of one workgroup per CU"
    h, v, r0 = operands(dev, dtype, n, seed=len(size) + n % 97)
    hb, vb, rb = (torch.from_numpy(x).to(dev) for x in (h, v, r0))
    scalars = [(1.0, 0.0), (2.0, -3.0)]
    if dtype == torch.float32:
        scalars.append((np.float32(0.5), 0.25))
    for off in (0, 1):
        ht, vt = hb[off:off + n], vb[off:off + n]
        H = lo.opHouseholder(ht)
        for alpha, beta in scalars:
            res = rb.clone()[off:off + n]
            assert apply(lo, ctx, res, H, vt, alpha, beta, fused=1) == 2, (size, off, alpha, beta)
            res3 = rb.clone()[off:off + n]
            assert apply(lo, ctx, res3, H, vt, alpha, beta, fused=0) == 3, (size, off, alpha, beta)
            assert torch.equal(res, res3), (size, off, alpha, beta)
            fl = oracle.scalar_flags(NP[dtype], alpha, beta)
            want = oracle.householder_mul(r0[off:off + n].copy(), h[off:off + n], v[off:off + n], float(alpha), float(beta),
                                          flags=fl)
            err = rel(res.cpu().numpy(), want)
            print(f"{dtype} {size} n={n} off={off} alpha={alpha} beta={beta}: rel err {err:.3e}")
            assert err <= TOL[dtype], (size, off, alpha, beta, err)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_res_alone_misaligned_falls_back(lo, dev, dtype):
    ctx = lo.get_ctx(dev)
    n = sizes(ctx, dtype)["ragged"]
    h, v, r0 = operands(dev, dtype, n, seed=3)
    hb, vb, rb = (torch.from_numpy(x).to(dev) for x in (h, v, r0))
    H = lo.opHouseholder(hb[:n])
    res = rb.clone()[1:n + 1]                                           # h and v aligned, res one element off
    assert apply(lo, ctx, res, H, vb[:n], 2.0, -3.0, fused=1) == 3
    want = oracle.householder_mul(r0[1:n + 1].copy(), h[:n], v[:n], 2.0, -3.0)
    assert rel(res.cpu().numpy(), want) <= TOL[dtype]


def test_res_aliasing_h(lo, dev):
    ctx = lo.get_ctx(dev)
    n = sizes(ctx, torch.float64)["ragged"]
    h, v, _ = operands(dev, torch.float64, n, seed=4)
    for off in (0, 1):
        for alpha, beta in ((1.0, 0.0), (2.0, -3.0)):
            ht = torch.from_numpy(h).to(dev)[off:off + n]
            vt = torch.from_numpy(v).to(dev)[off:off + n]
            assert apply(lo, ctx, ht, lo.opHouseholder(ht), vt, alpha, beta, fused=1) == 2
            h3 = torch.from_numpy(h).to(dev)[off:off + n]
            apply(lo, ctx, h3, lo.opHouseholder(h3), vt, alpha, beta, fused=0)
            assert torch.equal(ht, h3), (off, alpha, beta)
            want = oracle.householder_mul(h[off:off + n].copy(), h[off:off + n], v[off:off + n], alpha, beta)
            assert rel(ht.cpu().numpy(), want) <= 1e-12


def test_nan_poisons_every_element_and_the_next_apply_is_clean(lo, dev):
    ctx = lo.get_ctx(dev)
    n = sizes(ctx, torch.float64)["two_rounds"]
    h, v, _ = operands(dev, torch.float64, n, seed=5)
    ht, vt = torch.from_numpy(h[:n]).to(dev), torch.from_numpy(v[:n]).to(dev)
    H = lo.opHouseholder(ht)
    res = torch.zeros(n, dtype=torch.float64, device=dev)
    for where in (12345, n - 1):                                        # in a streamed round, in the scalar tail
        keep = float(vt[where])
        vt[where] = float("nan")
        assert apply(lo, ctx, res, H, vt, 1.0, 0.0, fused=1) == 2
        assert bool(torch.isnan(res).all()), where
        vt[where] = keep
        assert apply(lo, ctx, res, H, vt, 1.0, 0.0, fused=1) == 2
        assert rel(res.cpu().numpy(), oracle.householder_mul(np.empty(n), h[:n], v[:n], 1.0, 0.0)) <= 1e-12


def test_graph_replay(lo, dev):
    ctx = lo.get_ctx(dev)
    n = sizes(ctx, torch.float64)["two_rounds"]
    h, v, _ = operands(dev, torch.float64, n, seed=6)
    ht, vt = torch.from_numpy(h[:n]).to(dev), torch.from_numpy(v[:n]).to(dev)
    res = torch.empty(n, dtype=torch.float64, device=dev)
    with ctx.tuned(house_fused=1, **FORCE):
        g = lo.capture_mul(res, lo.opHouseholder(ht), vt, 1.0, 0.0)
        assert g.info()["nodes"] == 2                                   # kept dot launch + update launch
    for k in range(5):
        vt.mul_(1.0 + 0.1 * k)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want = oracle.householder_mul(np.empty(n), h[:n], vt.cpu().numpy(), 1.0, 0.0)
        assert rel(res.cpu().numpy(), want) <= 1e-12, k


def test_alternating_with_the_single_launch_form_shares_the_slots(lo, dev):
    """Both forms exchange their partials through the same two slot sets and epoch word."""
    ctx = lo.get_ctx(dev)
    n, m = sizes(ctx, torch.float64)["two_rounds"], 70_001
    h, v, _ = operands(dev, torch.float64, n, seed=7)
    ht, vt = torch.from_numpy(h[:n]).to(dev), torch.from_numpy(v[:n]).to(dev)
    hs, vs = torch.from_numpy(h[:m] / np.linalg.norm(h[:m])).to(dev), torch.from_numpy(v[:m]).to(dev)
    H, Hs = lo.opHouseholder(ht), lo.opHouseholder(hs)
    res, ress = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(m, dtype=torch.float64, device=dev)
    ref, refs = torch.empty_like(res), torch.empty_like(ress)
    assert apply(lo, ctx, ref, H, vt, 2.0, 0.0, fused=0) == 3
    apply(lo, ctx, refs, Hs, vs, 2.0, 0.0, fused=0)
    with ctx.tuned(house_fused=1, **FORCE):
        for k in range(200):
            res.zero_()
            ress.zero_()
            l0 = launches(lo)
            lo.mul(res, H, vt, 2.0, 0.0)
            lo.mul(ress, Hs, vs, 2.0, 0.0)
            assert launches(lo) - l0 == 3                               # kept form + update, single launch
            if k % 50 == 49:
                assert torch.equal(res, ref) and rel(ress.cpu().numpy(), refs.cpu().numpy()) <= 1e-12, k
    ctx.sync()
