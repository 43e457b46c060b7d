"""-m gpu: the tuning keys of a ctx (csrc/tune_keys.def) through mxlo_ctx_tune / mxlo_ctx_tune_get / mxlo_tune_key, and
`Context.tuned`, the scoped set-and-restore every other test file relies on. No kernels beyond ctx creation, except the
kron_fuse side effect at the end; every test but that one works on a Context of its own, not the session's."""
import numpy as np
import pytest
import torch

from test_gpu_kron import T, _fused_gate, _kron_launches, colmajor

pytestmark = pytest.mark.gpu

FLAGS = ("house_fused", "cherm_two_pass", "house_reverse")            # any value accepted, stored as value != 0
LISTS = {"gemm_tile": (-1, 0, 32, 64, 128), "herm_strip": (0, 1, 2, 8)}


@pytest.fixture()
def ctx(lo, dev):
    from linearoperators_jl_amd.device import Context
    return Context(dev.index)


@pytest.fixture(scope="module")
def table(lo):
    return lo._lib.tune_keys()


def refused(lo, ctx, key, value):
    with pytest.raises(lo.MxloError) as e:
        ctx.tune(key, value)
    return e.value.status == lo._lib.EINVAL


def test_fresh_ctx_holds_the_enumerated_defaults(ctx, table):
    assert {k: ctx.tune_get(k) for k, _, _, _ in table} == {k: d for k, d, _, _ in table}


def test_lowest_and_highest_are_accepted_and_read_back(ctx, table):
    num_cu = ctx.info()["num_cu"]
    for key, _, lo_, hi in table:
        if key == "red_blocks_per_cu":                                # highest: value x CUs <= the enumerated (static) bound
            lo_, hi = 1, hi // num_cu
        for val in (lo_, hi):
            ctx.tune(key, val)
            assert ctx.tune_get(key) == val, (key, val)


def test_outside_the_range_is_einval_and_changes_nothing(lo, ctx, table):
    num_cu = ctx.info()["num_cu"]
    for key, default, lo_, hi in table:
        if key in FLAGS:
            continue
        if key == "red_blocks_per_cu":
            hi //= num_cu
        for val in (lo_ - 1, hi + 1):
            if not -(1 << 63) <= val < (1 << 63):                     # no int64 beyond an unbounded end
                continue
            assert refused(lo, ctx, key, val), (key, val)
            assert ctx.tune_get(key) == default, (key, val)
    for key, val in (("gemm_tile", 48), ("herm_strip", 3)):           # inside lowest .. highest, not in the list
        assert refused(lo, ctx, key, val), (key, val)
        assert ctx.tune_get(key) == 0, key                            # (the default of both)
    for key, vals in LISTS.items():
        for val in vals:
            ctx.tune(key, val)
            assert ctx.tune_get(key) == val


def test_flag_keys_store_one_for_any_nonzero_value(ctx):
    for key in FLAGS:
        for val, want in ((7, 1), (0, 0), (-3, 1)):
            ctx.tune(key, val)
            assert ctx.tune_get(key) == want, (key, val)


def test_unknown_key_is_einval_for_setter_and_getter(lo, ctx):
    assert refused(lo, ctx, "no_such_key", 1)
    with pytest.raises(lo.MxloError) as e:
        ctx.tune_get("no_such_key")
    assert e.value.status == lo._lib.EINVAL
    import ctypes as C
    L = lo._lib.lib()
    assert L.mxlo_ctx_tune_get(ctx.handle, b"house_fused", None) == lo._lib.EINVAL
    assert L.mxlo_ctx_tune_get(ctx.handle, None, C.byref(C.c_int64())) == lo._lib.EINVAL
    assert L.mxlo_ctx_tune_get(None, b"house_fused", C.byref(C.c_int64())) == lo._lib.EINVAL


def test_tuned_restores_after_a_normal_exit(ctx):
    with ctx.tuned(house_fused=0, fused_timeout_ms=50, nt_min_bytes=1 << 40) as inside:
        assert inside is ctx
        assert (ctx.tune_get("house_fused"), ctx.tune_get("fused_timeout_ms"), ctx.tune_get("nt_min_bytes")) == (0, 50, 1 << 40)
    assert (ctx.tune_get("house_fused"), ctx.tune_get("fused_timeout_ms"), ctx.tune_get("nt_min_bytes")) == (1, 2000, 256 << 20)
    with ctx.tuned():                                                 # no keys: nothing to do
        pass


def test_tuned_restores_after_an_exception_and_after_pytest_fail(ctx):
    with pytest.raises(ZeroDivisionError):
        with ctx.tuned(qn_persist=0, herm_strip=8):
            assert ctx.tune_get("herm_strip") == 8
            1 / 0
    assert (ctx.tune_get("qn_persist"), ctx.tune_get("herm_strip")) == (1, 0)
    with pytest.raises(pytest.fail.Exception):
        with ctx.tuned(qn_persist=0):
            pytest.fail("inside the block")
    assert ctx.tune_get("qn_persist") == 1


def test_tuned_restores_what_the_block_changed_by_hand(ctx):
    """... as the library's fault path does with the single-launch forms."""
    with ctx.tuned(kron_fuse=1, fused_debug_drop=3):
        ctx.tune("kron_fuse", 0)
        ctx.tune("fused_debug_drop", -1)
        ctx.tune("herm_single", 0)                                    # not named: not restored
    assert (ctx.tune_get("kron_fuse"), ctx.tune_get("fused_debug_drop"), ctx.tune_get("herm_single")) == (1, -1, 0)


def test_tuned_nests(ctx):
    with ctx.tuned(push_fused=0, dots_max_nc=10):
        with ctx.tuned(push_fused=1):
            assert (ctx.tune_get("push_fused"), ctx.tune_get("dots_max_nc")) == (1, 10)
            with ctx.tuned(dots_max_nc=5, push_fused=0):
                assert (ctx.tune_get("push_fused"), ctx.tune_get("dots_max_nc")) == (0, 5)
            assert (ctx.tune_get("push_fused"), ctx.tune_get("dots_max_nc")) == (1, 10)
        assert (ctx.tune_get("push_fused"), ctx.tune_get("dots_max_nc")) == (0, 10)
    assert (ctx.tune_get("push_fused"), ctx.tune_get("dots_max_nc")) == (1, 20)


def test_tuned_entry_that_is_refused_sets_nothing(lo, ctx):
    with pytest.raises(lo.MxloError):
        with ctx.tuned(house_fused=0, gemm_tile=48):                  # the second set is refused: the first is undone
            pytest.fail("the block must not run")
    assert (ctx.tune_get("house_fused"), ctx.tune_get("gemm_tile")) == (1, 0)
    with pytest.raises(lo.MxloError):
        with ctx.tuned(house_fused=0, no_such_key=1):                 # refused before anything is set
            pytest.fail("the block must not run")
    assert ctx.tune_get("house_fused") == 1


def test_tuned_restores_every_key_even_if_one_restore_raises(lo, ctx, monkeypatch):
    real = ctx.tune

    def tune(key, value):
        if key == "herm_order" and value == 1:                        # the restore of the middle key fails
            raise lo.MxloError(lo._lib.EHIP, "injected")
        real(key, value)
    with pytest.raises(lo.MxloError, match="injected"):
        with ctx.tuned(house_fused=0, herm_order=0, qn_persist=0):
            monkeypatch.setattr(ctx, "tune", tune)
    monkeypatch.undo()
    assert (ctx.tune_get("house_fused"), ctx.tune_get("herm_order"), ctx.tune_get("qn_persist")) == (1, 0, 1)


def test_leaving_the_no_wait_kron_mode_through_tuned_rearms_the_counters(lo, dev):
    """`kron_fuse` = 2 (no wait: wrong results, counters left in any state) entered and left by a `tuned` block: the
    one-launch apply that follows has the bits of the two-launch form. The smallest shape of test_gpu_kron.py's
    comparison (64 x 64 factors: 16 workgroups of the one-launch form) on the session's ctx, which the applies use."""
    ctx = lo.get_ctx(dev)
    shape = ((64, 64), (64, 64))
    rng = np.random.default_rng(64)
    A, B = rng.uniform(-1, 1, shape[0]), rng.uniform(-1, 1, shape[1])
    K = lo.kron(colmajor(A, dev), colmajor(B, dev))
    x = T(rng.uniform(-1, 1, 64 * 64), dev)
    want, got = torch.empty_like(x), torch.full_like(x, float("nan"))
    with ctx.tuned(kron_fuse=0):
        lo.mul(want, K, x)
    with ctx.tuned(kron_fuse=1):
        gate = _fused_gate(shape, torch.float64, ctx.info()["num_cu"])
        assert gate, "the smallest comparison shape is one the gate admits"
        fused = _kron_launches(lo, got, K, x) == 1                    # (also allocates the counters)
        with ctx.tuned(kron_fuse=2):
            for _ in range(3):
                lo.mul(got, K, x)
        assert ctx.tune_get("kron_fuse") == 1
        for _ in range(3):
            got.fill_(float("nan"))
            assert _kron_launches(lo, got, K, x) == (1 if fused else 2)
            assert torch.equal(got, want)
    torch.cuda.synchronize()
