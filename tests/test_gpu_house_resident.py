"""The resident slice of h in the kept form of the Householder apply (csrc/house_keep.h, csrc/house_keep_plan.h): q of
every 16 chunks of h are loaded with the default cache policy in the dot launch and in the update launch over the
prefix, everything else stays nontemporal. A cache policy cannot change a bit; these tests are there to catch an index or
predicate slip between the two kernels and a wrong fallback. The kept form is forced at small n with the keys of
tests/test_gpu_house_keep.py, and nt_min_bytes — the key the slice's target is a fraction of — is set near the size of h
so that q lands on 0, on a middle value and on 16. Every result is compared bit for bit with the three-launch path
(house_fused = 0 under the same keys) and with the oracle."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

NP = {torch.float64: np.float64, torch.float32: np.float32}
TOL = {torch.float64: 1e-12, torch.float32: 1e-5}
FORCE = dict(house_inline_n=0, house_fused_per_cu=1)
RESIDENT_NUM = 14                 # kHouseResidentNum: the target is RESIDENT_NUM / 16 of nt_min_bytes
SCALARS = ((1.0, 0.0), (2.0, -3.0))
SIZES = {"two_rounds": lambda R: 4 * R + 1, "one_streamed_round": lambda R: 19 * R, "ragged": lambda R: 21 * R + 12345}


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) or 1.0))


def launches(lo):
    a = (C.c_int64 * 12)()
    lo._lib.call("mxlo_debug_counters", a)
    return a[10]


def resident_q(h_bytes, nt_min_bytes):
    """house_resident_q(h_bytes, nt_min_bytes / 16 * kHouseResidentNum) of csrc/house_keep_plan.h."""
    target = nt_min_bytes // 16 * RESIDENT_NUM
    if target <= 0:
        return 0
    return 16 if h_bytes <= target else target // ((h_bytes + 15) // 16)


def nt_min_for(case, h_bytes):
    """nt_min_bytes for which the kept form engages (2 h_bytes >= nt_min_bytes) and q is none / a middle value / all."""
    return {"q0": 0, "qmid": h_bytes * 2 // 3, "q16": h_bytes * 3 // 2}[case]


@functools.lru_cache(maxsize=None)
def operands(dtype, n):
    """(h, v, r0) as read-only numpy arrays of n + 1 elements: views [off:off + n] give both 16-byte phases."""
    rng = np.random.default_rng(n % 9973)
    h = rng.standard_normal(n + 1).astype(NP[dtype])
    h /= np.linalg.norm(h.astype(np.float64))
    v = rng.uniform(-1, 1, n + 1).astype(NP[dtype])
    r0 = rng.uniform(-1, 1, n + 1).astype(NP[dtype])
    for x in (h, v, r0):
        x.setflags(write=False)
    return h, v, r0


@functools.lru_cache(maxsize=None)
def want(dtype, n, off, alpha, beta):
    h, v, r0 = operands(dtype, n)
    out = oracle.householder_mul(r0[off:off + n].copy(), h[off:off + n], v[off:off + n], alpha, beta,
                                 flags=oracle.scalar_flags(NP[dtype], alpha, beta))
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("case", ["q0", "qmid", "q16"])
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_resident_slice_matches_three_launch_path_and_oracle(lo, dev, dtype, size, case):
    ctx = lo.get_ctx(dev)
    esize = torch.empty(0, dtype=dtype).element_size()
    R = ctx.info()["num_cu"] * 1024 * (16 // esize)           # elements of one round of the dot launch
    n = SIZES[size](R)
    nt_min = nt_min_for(case, n * esize)
    q = resident_q(n * esize, nt_min)
    assert {"q0": q == 0, "qmid": 0 < q < 16, "q16": q == 16}[case], (case, q)
    assert 2 * n * esize >= nt_min and n > 4 * R
    h, v, r0 = operands(dtype, n)
    hb, vb, rb = (torch.from_numpy(x.copy()).to(dev) for x in (h, v, r0))
    for off in (0, 1):
        ht, vt = hb[off:off + n], vb[off:off + n]
        H = lo.opHouseholder(ht)
        for alpha, beta in SCALARS:
            got = {}
            for fused, nlaunch in ((1, 2), (0, 3)):
                res = rb.clone()[off:off + n]
                with ctx.tuned(house_fused=fused, nt_min_bytes=nt_min, **FORCE):
                    l0 = launches(lo)
                    lo.mul(res, H, vt, alpha, beta)
                    assert launches(lo) - l0 == nlaunch, (size, case, off, alpha, beta, fused)
                got[fused] = res
            assert torch.equal(got[1], got[0]), (size, case, off, alpha, beta)
            err = rel(got[1].cpu().numpy(), want(dtype, n, off, alpha, beta))
            print(f"{dtype} {size} n={n} q={q} off={off} alpha={alpha} beta={beta}: rel err {err:.3e}")
            assert err <= TOL[dtype], (size, case, off, alpha, beta, err)
