"""The block form of opQR's apply on the device (`mxlo_qr_mul_block`, qr_reflect_block_kernel in csrc/linalg.hip): `mul!` with
an n x k matrix operand runs the chain of ONE vector apply per group of 8 columns, and column j of the result is the vector
apply of column j BIT FOR BIT.

Matrices, seeds, the factored operators and the accuracy checks are those of tests/test_gpu_qr.py (simple_matrix made
rectangular, condition number 2), shared through that module so that every (shape, dtype, orientation) is factored once.
Shapes (mf, nf): one entry and a ragged tiny one; exactly one block, then a ragged row chunk; 2 and 3 block columns;
(40001, 5) has more row chunks than the 512 workgroups of a pass, so they stride, and no column start is 16-byte aligned.
k runs over one column, a partial group, 7 | 8 | 9 around the group size and 17 = two groups and one column.

The accuracy bound is mf eps(T), derived in tests/test_gpu_qr.py (Higham, Thms 19.4 and 20.3, constants and the factor n
dropped); LAPACK's own solve stays at or below 0.23 of it for these matrices. It guards against a bit-for-bit test that
compares two equally wrong paths."""
import gc

import numpy as np
import pytest
import torch

import test_gpu_qr as q

gpu = pytest.mark.gpu
KS = (1, 2, 7, 8, 9, 17)
KMAX = max(KS)
F64, F32 = torch.float64, torch.float32
CASES = [((mf, nf), F64, KS) for mf, nf in ((1, 1), (5, 3), (64, 64), (65, 64), (65, 65), (129, 65), (200, 129), (40001, 5))]
CASES += [(s, F32, (2, 9)) for s in ((65, 64), (200, 129), (40001, 5))]
CASE_IDS = [f"{s[0]}x{s[1]}-{'f64' if d is F64 else 'f32'}" for s, d, _ in CASES]
BITS = {F64: torch.int64, F32: torch.int32}
NAN = float("nan")


def modes(lo, op):
    """(operator, MXLO op_mode of the C entry point) for op and its transpose: a tall A's prod! is the N mode"""
    n, t = lo._lib.OP_N, lo._lib.OP_T
    return ((op, n if op._tall else t), (lo.transpose(op), t if op._tall else n))


def padded(rows, cols, ld, dtype, dev, fill=NAN):
    """a column-major rows x cols view in a leading dimension ld inside a buffer that holds `fill` everywhere"""
    buf = torch.full((ld * cols,), fill, dtype=dtype, device=dev)
    return buf, buf.as_strided((rows, cols), (1, ld))


def same_bits(a, b):
    return torch.equal(a.view(BITS[a.dtype]), b.view(BITS[b.dtype]))


def block_mul(lo, leaf, mode, R, ldr, V, ldv, k, alpha, beta):
    """the C entry point itself, with the operator's own factor"""
    W, tfac, dinv, work = leaf._factor
    mf, nf = W.shape
    return lo._lib.call("mxlo_qr_mul_block", lo.linalg.ctx_of(R).handle, lo.linalg.dtype_code(W.dtype), R.data_ptr(), ldr, W.data_ptr(),
                        W.stride(1), mf, nf, tfac.data_ptr(), dinv.data_ptr(), work.data_ptr(), V.data_ptr(), ldv, k, mode,
                        float(alpha), float(beta))


def operands(nin, nout, dtype, dev, seed):
    """V (nin x KMAX) and R0 (nout x KMAX), dense column-major, Gaussians rounded to the device precision"""
    rng = np.random.default_rng(seed)
    V = torch.from_numpy(rng.standard_normal((KMAX, nin))).to(dtype).to(dev).t()
    R0 = torch.from_numpy(rng.standard_normal((KMAX, nout))).to(dtype).to(dev).t()
    return V, R0


# ------------------------------------------------------------------------------------------------ 1. bit for bit
@gpu
@pytest.mark.parametrize("wide", [False, True], ids=["tall", "wide"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_column_of_a_block_apply_is_its_vector_apply_bit_for_bit(lo, dev, case, wide):
    shape, dtype, ks = case
    leaf = q.factored(lo, dev, shape, dtype, wide=wide)
    for w, mode in modes(lo, leaf):
        nout, nin = lo.size(w, 1), lo.size(w, 2)
        V, Rg = operands(nin, nout, dtype, dev, 7400 + 7 * shape[0] + shape[1])
        for alpha, beta in ((1.0, 0.0), (2.0, -0.5)):
            R0 = Rg if beta else torch.full_like(Rg, NAN)                  # with beta == 0 res is not read
            want = []                                                      # the vector applies, once for every k
            for j in range(max(ks)):
                r = R0[:, j].clone()
                lo.mul(r, w, V[:, j].clone(), alpha, beta)
                want.append(r)
            assert all(torch.isfinite(r).all() for r in want)
            for k in ks:
                ldr, ldv = nout + 5, nin + 3
                Rbuf, R = padded(nout, k + 2, ldr, dtype, dev)             # two columns more than the apply is given
                Vbuf, Vk = padded(nin, k, ldv, dtype, dev)
                R[:, :k].copy_(R0[:, :k])
                Vk.copy_(V[:, :k])
                before, vbefore = Rbuf.clone(), Vbuf.clone()
                if k > 1:
                    lo.mul(R[:, :k], w, Vk, alpha, beta)
                else:                                                      # mul! hands one column to the vector entry point
                    block_mul(lo, leaf, mode, R, ldr, Vk, ldv, 1, alpha, beta)
                for j in range(k):
                    assert torch.equal(R[:, j], want[j]), (shape, mode, k, j, alpha, beta)
                assert same_bits(Vbuf, vbefore)
                after = Rbuf.clone()
                for b in (after, before):                                  # everything but the k columns: unchanged bitwise
                    b.as_strided((nout, k), (1, ldr)).zero_()
                assert same_bits(after, before), (shape, mode, k)


# ------------------------------------------------------------------------------------------------ 2. launches
@gpu
def test_a_block_apply_is_one_chain_per_group_and_only_launches(lo, dev):
    dtype = F64
    for k in (8, 9, 17):
        deltas = []
        for shape in ((129, 65), (2049, 65)):
            leaf = q.factored(lo, dev, shape, dtype)
            for w, _ in modes(lo, leaf):
                V = torch.ones((k, lo.size(w, 2)), dtype=dtype, device=dev).t()
                R = torch.zeros((k, lo.size(w, 1)), dtype=dtype, device=dev).t()
                lo.mul(R, w, V, 2.0, -0.5)
                gc.collect()
                torch.cuda.synchronize()
                a = q.counters(lo)
                lo.mul(R, w, V, 2.0, -0.5)
                b = q.counters(lo)
                torch.cuda.synchronize()
                d = {key: b[key] - a[key] for key in q.NAMES}
                assert d["launch"] == lo.linalg.qr_block_launches(shape[1], k), (k, shape, d)
                assert not {key: x for key, x in d.items() if key != "launch" and x}, d
                deltas.append(d["launch"])
        assert len(set(deltas)) == 1, (k, deltas)                          # the same for 129 and 2049 rows, in both modes


# ------------------------------------------------------------------------------------------------ 3. aliasing
@gpu
def test_res_may_be_v_as_the_same_matrix_and_every_other_overlap_is_refused(lo, dev):
    dtype, n, k = F64, 65, 9
    leaf = q.factored(lo, dev, (n, n), dtype)
    for w, _ in modes(lo, leaf):
        V, _ = operands(n, n, dtype, dev, 7)
        V = V[:, :k]
        out = torch.zeros((k, n), dtype=dtype, device=dev).t()
        lo.mul(out, w, V, 2.0, 0.0)
        X = V.clone(memory_format=torch.preserve_format)
        assert X.stride() == (1, n)
        lo.mul(X, w, X, 2.0, 0.0)
        assert torch.equal(X, out)
        buf = torch.ones((n + 1) * k + 1, dtype=dtype, device=dev)
        a, b = buf.as_strided((n, k), (1, n)), buf.as_strided((n, k), (1, n + 1))
        with pytest.raises(lo.MxloError, match="overlaps"):               # the same pointer, another leading dimension
            lo.mul(b, w, a, 1.0, 0.0)
        with pytest.raises(lo.MxloError, match="overlaps"):               # a partial overlap
            lo.mul(buf[1:].as_strided((n, k), (1, n)), w, a, 1.0, 0.0)
        assert torch.equal(buf, torch.ones_like(buf))                      # nothing was launched
        W = leaf._factor[0]
        keep = W.clone(memory_format=torch.preserve_format)
        with pytest.raises(lo.MxloError, match="overlaps"):               # V inside the factor
            lo.mul(out, w, W[:, :k], 1.0, 0.0)
        assert same_bits(W.t().contiguous(), keep.t().contiguous())


# ------------------------------------------------------------------------------------------------ 4. containment
@gpu
def test_a_nan_and_an_inf_in_one_column_reach_no_other_column(lo, dev):
    dtype, k = F64, 9
    leaf = q.factored(lo, dev, (129, 65), dtype)
    for w, _ in modes(lo, leaf):
        V, R0 = operands(lo.size(w, 2), lo.size(w, 1), dtype, dev, 17)
        V, R0 = V[:, :k], R0[:, :k]
        clean = R0.clone(memory_format=torch.preserve_format)
        lo.mul(clean, w, V, 2.0, -0.5)
        bad = V.clone(memory_format=torch.preserve_format)
        bad[3, 3] = NAN
        bad[5, 3] = float("inf")
        got = R0.clone(memory_format=torch.preserve_format)
        lo.mul(got, w, bad, 2.0, -0.5)
        for j in range(k):
            if j != 3:
                assert torch.equal(got[:, j], clean[:, j]), j
        assert not torch.isfinite(got[:, 3]).all()


# ------------------------------------------------------------------------------------------------ 5. capture
@gpu
def test_a_captured_block_apply_replays_to_the_bits_of_the_eager_one(lo, dev):
    dtype, k = F64, 9
    leaf = q.factored(lo, dev, (129, 65), dtype)
    for w, _ in modes(lo, leaf):
        V, R0 = operands(lo.size(w, 2), lo.size(w, 1), dtype, dev, 19)
        V, R0 = V[:, :k], R0[:, :k]
        eager = R0.clone(memory_format=torch.preserve_format)
        lo.mul(eager, w, V, 2.0, -0.5)
        res = R0.clone(memory_format=torch.preserve_format)
        g = lo.capture_mul(res, w, V, 2.0, -0.5)
        res.copy_(R0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(res, eager)


# ------------------------------------------------------------------------------------------------ 6. accuracy
@gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(200, 129), (40001, 5)], ids=["200x129", "40001x5"])
def test_every_column_of_a_block_apply_solves_its_problem(lo, dev, shape, dtype):
    k = 9
    A, _, _, nA = q.problem(*shape, q.NP[dtype])
    eps = float(torch.finfo(dtype).eps)
    m, n = shape
    op = q.factored(lo, dev, shape, dtype)
    V, U = operands(m, n, dtype, dev, 23)
    X = torch.full((k, n), NAN, dtype=dtype, device=dev).t()
    lo.mul(X, op, V[:, :k])
    Y = torch.full((k, m), NAN, dtype=dtype, device=dev).t()
    lo.mul(Y, lo.transpose(op), U[:, :k])
    Vh, Uh, Xh, Yh = q.host(V), q.host(U), q.host(X), q.host(Y)
    assert np.isfinite(Xh).all() and np.isfinite(Yh).all()
    for j in range(k):
        q.check_least_squares(f"block {shape} {dtype} column {j}", A, nA, Vh[:, j], Xh[:, j], eps)
        q.check_minimum_norm(f"block {shape} {dtype} column {j}", A, nA, Uh[:, j], Yh[:, j], eps)


# ------------------------------------------------------------------------------------------------ 7. the ABI directly
@gpu
def test_the_entry_point_itself_on_no_columns_a_null_operand_and_a_short_leading_dimension(lo, dev):
    dtype, (m, n) = F64, (129, 65)
    leaf = q.factored(lo, dev, (m, n), dtype)
    V = torch.ones((2, m), dtype=dtype, device=dev).t()
    R = torch.zeros((2, n), dtype=dtype, device=dev).t()
    torch.cuda.synchronize()
    a = q.counters(lo)
    block_mul(lo, leaf, lo._lib.OP_N, R, n, V, m, 0, 1.0, 0.0)                       # MXLO_OK: anything else raises
    b = q.counters(lo)
    assert a == b                                                          # k == 0: nothing is launched
    assert not R.any()

    class Null:
        @staticmethod
        def data_ptr():
            return None

    with pytest.raises(lo.MxloError) as ei:
        block_mul(lo, leaf, lo._lib.OP_N, R, n, Null, m, 2, 1.0, 0.0)
    assert ei.value.status == lo._lib.EINVAL
    for mode, ldr, ldv in ((lo._lib.OP_N, n - 1, m), (lo._lib.OP_T, m - 1, n)):
        with pytest.raises(lo.MxloError) as ei:
            block_mul(lo, leaf, mode, R, ldr, V, ldv, 2, 1.0, 0.0)
        assert ei.value.status == lo._lib.ESHAPE
    assert not R.any()
