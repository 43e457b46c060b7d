"""CPU: the cases of tests/linalg_fuzz_cases.py are deterministic, reach what they are meant to reach, and cannot fail a correct
kernel: LAPACK in the case's precision (scipy) solves every seed's problem — every seed tests/test_gpu_linalg_fuzz.py runs, by
default and under MXLO_LINFUZZ_SEEDS — within 0.5 of every bound the GPU test holds the device to, and finds the drawn rank with
a factor of 20 on both sides of the threshold. No device call anywhere in this file.

References. chol: cho_factor / cho_solve; lu: lu_factor / lu_solve; lower, upper: solve_triangular; ldl: LAPACK's symmetric
indefinite solve (sytrf, Bunch-Kaufman: scipy.linalg.solve(assume_a="sym")) — LAPACK has no unpivoted LDL', and the bound
n eps rho with rho >= 1 is the weaker one; qr: geqrf; qrp: test_gpu_qrp.lapack_basic; pinv: test_gpu_pinv.host_cod.

The distance of a minimum-norm solution from range(F) is taken for mf > nf only, against an orthonormal basis (a Float64 QR for the
full-rank qr family, test_gpu_qrp.range_basis for qrp and pinv), never through lstsq: linalg_fuzz_cases.ratios says why.

Worst reference / bound, which the test prints per family, metric and precision — over the 320 default seeds / over 4000 seeds:
chol 0.07 / 0.12, lower 0.05 / 0.09, upper 0.06 / 0.10, lu 0.07 / 0.17, ldl 0.10 / 0.10 (the bound is n eps rho), qr least squares
0.02 / 0.12, minimum-norm residual 0.13 / 0.36, range 0.26 / 0.26; qrp least squares 0.03 / 0.10, consistent wide residual 0.05 /
0.37, range 0.06 / 0.26; pinv least squares 0.05 / 0.11, row space 0.16 / 0.43, range 0.05 / 0.21. ldl and pinv, which had not
been measured before, needed no larger smallest size. Rank margins over 4000 seeds: |R_rr| at least 145 thresholds, |R_r+1,r+1|
at most 0.043 of one. The whole file takes about 13 s; the cases of 32833 and 40001 rows take 0.1 .. 0.9 s each."""
import time

import numpy as np
import pytest

import linalg_fuzz_cases as fz
import test_gpu_pinv as t_pinv
import test_gpu_qrp as t_qrp

HALF = 0.5
MARGIN = 20.0


@pytest.fixture(scope="module")
def cases():
    return [fz.case(s) for s in fz.seeds()]


def equal_cases(a, b):
    da, db = vars(a), vars(b)
    assert da.keys() == db.keys()
    for key, x in da.items():
        y = db[key]
        if isinstance(x, np.ndarray):
            if not (x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=True)):
                return False
        elif x != y:
            return False
    return True


# ------------------------------------------------------------------------------------------------ 1. determinism
def test_a_case_is_a_function_of_its_seed(cases):
    for c in cases:
        if c.mf <= fz.BIG_ROWS:
            assert equal_cases(c, fz.case(c.seed)), c.seed
    big = next(c for c in cases if c.mf > fz.BIG_ROWS)
    assert equal_cases(big, fz.case(big.seed))
    for c in cases:                                         # the storage is a function of the case
        if c.mf <= fz.BIG_ROWS:
            a, b = fz.matrix_storage(c), fz.matrix_storage(c)
            assert np.array_equal(a[0], b[0], equal_nan=True) and a[1:] == b[1:]


def test_the_environment_variable_only_extends_the_list(monkeypatch):
    monkeypatch.delenv("MXLO_LINFUZZ_SEEDS", raising=False)
    default = list(fz.seeds())
    assert default == list(range(fz.DEFAULT_SEEDS)) and fz.DEFAULT_SEEDS >= 2 * len(fz.FORCED)
    monkeypatch.setenv("MXLO_LINFUZZ_SEEDS", str(fz.DEFAULT_SEEDS + 7))
    longer = list(fz.seeds())
    assert longer[:len(default)] == default and len(longer) == len(default) + 7
    assert equal_cases(fz.case(60), fz.case(60))            # and a case does not look at the variable


# ------------------------------------------------------------------------------------------------ 2. the storage helpers
def test_the_storage_puts_the_matrix_where_it_says_and_nan_elsewhere(cases):
    for c in cases:
        if c.mf > fz.BIG_ROWS:
            continue
        buf, shape, strides, offset = fz.matrix_storage(c)
        assert buf.dtype == c.npd and shape == c.A.shape
        assert np.array_equal(fz.window(buf, shape, strides, offset), c.A)
        rest = np.ones(buf.shape, dtype=bool)
        fz.window(rest, shape, strides, offset)[...] = False
        assert np.isnan(buf[rest]).all() and rest.sum() == buf.size - c.A.size
        if c.storage == "strided":
            assert strides[0] == 2 and strides[1] >= 4 * shape[0]
        else:
            assert offset == c.off and (offset > 0) == (c.storage == "offset")
            assert strides == ((shape[1] + c.pad, 1) if c.rowmajor else (1, shape[0] + c.pad))
        V, vshape, vstrides, voff = fz.operand_storage(c.V.astype(c.npd), c.ldv, c.offv, np.nan)
        assert np.array_equal(fz.window(V, vshape, vstrides, voff), c.V) and voff == fz.GUARD + c.offv
        assert fz.outside(V, vshape, vstrides, voff).size == V.size - c.V.size >= 2 * fz.GUARD


# ------------------------------------------------------------------------------------------------ 3. coverage
def test_the_default_seeds_reach_what_they_are_meant_to_reach():
    """every count below is at least 3 over the default seeds; every forced shape is forced exactly once per precision, and the
    shapes above BIG_ROWS occur nowhere else"""
    cs = [fz.case(s) for s in range(fz.DEFAULT_SEEDS)]
    counts = {}

    def count(*key):
        counts[key] = counts.get(key, 0) + 1

    for c in cs:
        f = c.family
        count("family", f, c.npd.__name__)
        count("storage", f, c.storage)
        count("wrapper", c.wrapper)
        count("scalars", c.scalars_index)
        count("operand", "vector" if c.vector else "matrix")
        if not c.vector:
            count("group", "ragged" if c.k % 8 else "full")
            if c.ldr != c.ldv:
                count("ldr != ldv")
        if c.refine:
            count("refine", f)
        if f in ("qrp", "pinv"):
            count("rtol", "default" if c.rtol is None else "explicit")
            count("rank", "full" if c.rank == c.nf else "deficient")
        if not c.square:
            count("orientation", f, "wide" if c.wide else "tall")
            count("mode", f, "lsq" if c.lsq else "minimum norm")
        if c.alias:
            count("alias")
    want = ([("family", f, p) for f in fz.FAMILIES for p in ("float64", "float32")]
            + [("storage", f, s) for f in fz.FAMILIES for s in fz.STORAGES]
            + [("wrapper", w) for w in fz.WRAPPERS] + [("scalars", i) for i in range(len(fz.SCALARS))]
            + [("operand", "vector"), ("operand", "matrix"), ("group", "ragged"), ("group", "full"), ("ldr != ldv",)]
            + [("refine", f) for f in fz.REFINABLE] + [("rtol", "default"), ("rtol", "explicit")]
            + [("rank", "full"), ("rank", "deficient"), ("alias",)]
            + [(what, f, x) for f in fz.RECT for what, xs in (("orientation", ("tall", "wide")), ("mode", ("lsq", "minimum norm")))
               for x in xs])
    for key in sorted(counts, key=str):
        print(f"coverage {key}: {counts[key]}")
    short = {key: counts.get(key, 0) for key in want if counts.get(key, 0) < 3}
    assert not short, short
    assert all(c.k in (8, 16, 24) for c in cs if not c.vector and c.k % 8 == 0)
    for family, shape in fz.FORCED:
        for npd in (np.float64, np.float32):
            hits = [c for c in cs if c.family == family and c.shape == shape and c.npd is npd]
            # a later seed may draw one of the shapes 64 j + d again on its own; the rows above BIG_ROWS come once only
            assert sum(h.forced for h in hits) == 1 and hits[0].forced, (family, shape, npd.__name__)
            assert len(hits) == 1 or hits[0].mf <= fz.BIG_ROWS, (family, shape, npd.__name__)
    # the sizes: nothing below 8, nothing drawn above BIG_ROWS
    for c in cs:
        assert c.nf >= 8 and (c.forced or c.mf <= fz.BIG_ROWS), (c.seed, c.shape)
        assert c.family not in ("qrp", "pinv") or (1 <= c.rank <= c.nf and (c.rtol is not None or max(c.mf, c.nf) >= 96))


# ------------------------------------------------------------------------------------------------ 4. LAPACK within half the bounds
def reference(c):
    """the case's problem solved by LAPACK in the case's precision: the result as Float64, rows_out x k"""
    from scipy import linalg as sl
    npd = c.npd
    F, V = c.F.astype(npd), c.V.astype(npd)
    trans = 1 if c.transposed else 0
    if c.family == "chol":
        X = sl.cho_solve(sl.cho_factor(F), V)
    elif c.family == "ldl":
        X = sl.solve(F, V, assume_a="sym")
    elif c.family == "lu":
        X = sl.lu_solve(sl.lu_factor(F), V, trans=trans)
    elif c.family in ("lower", "upper"):
        X = sl.solve_triangular(F, V, lower=c.family == "lower", trans=trans)
    elif c.family == "qr":
        Q, R = sl.qr(F, mode="economic")
        X = sl.solve_triangular(R, Q.T @ V) if c.lsq else Q @ sl.solve_triangular(R, V, trans="T")
    else:
        if c.family == "qrp":
            rank, _, _, solve, solve_t = t_qrp.lapack_basic(c.F, npd, c.rtol)
        else:
            rank, solve, solve_t = t_pinv.host_cod(c.F, npd, c.rtol)
        assert rank == c.rank, (c.seed, c.shape, rank)
        X = np.stack([(solve if c.lsq else solve_t)(c.V[:, j]) for j in range(c.k)], axis=1)
    assert X.dtype == npd or c.family in ("qrp", "pinv")
    return np.asarray(X, dtype=np.float64).reshape(c.rows_out, c.k)


def test_lapack_in_the_cases_precision_stays_within_half_of_every_bound(cases):
    """No seed is dropped: a reference above 0.5 of a bound at some seed fails this test. The rows above BIG_ROWS are timed."""
    worst = {}
    for c in cases:
        t0 = time.perf_counter()
        X = reference(c)
        assert np.isfinite(X).all(), c.seed
        for name, ratio in fz.ratios(c, X).items():
            key = (c.family, name, c.npd.__name__)
            if ratio > worst.get(key, (0.0, None))[0]:
                worst[key] = (ratio, c.seed, c.shape)
            assert ratio <= HALF, (c.seed, c.family, c.shape, c.npd.__name__, name, ratio)
        if c.mf > fz.BIG_ROWS:
            print(f"seed {c.seed} {c.family} {c.shape} {c.npd.__name__} k={c.k}: {time.perf_counter() - t0:.2f} s")
    for key in sorted(worst):
        ratio, seed, shape = worst[key]
        print(f"reference / bound {key[0]} {key[1]} {key[2]}: {ratio:.3f} (seed {seed}, {shape})")
    assert {k[0] for k in worst} == set(fz.FAMILIES)


# ------------------------------------------------------------------------------------------------ 5. rank margins
def test_lapack_finds_the_drawn_rank_with_a_factor_of_twenty_on_both_sides(cases):
    above, below = {}, {}
    seen = set()
    for c in cases:
        key = (c.shape, c.npd, c.rtol)
        if c.family not in ("qrp", "pinv") or key in seen:
            continue
        seen.add(key)                                       # qrp and pinv share the matrices
        rank, d, _, _, _ = t_qrp.lapack_basic(c.F, c.npd, c.rtol)
        assert rank == c.rank, (c.seed, c.shape, rank)
        thr = c.rtol_value * d[0]
        kind = ("default" if c.rtol is None else "explicit", c.npd.__name__)
        hi = d[c.rank - 1] / thr
        assert hi >= MARGIN, (c.seed, c.shape, hi)
        above[kind] = min(above.get(kind, np.inf), hi)
        if c.rank < c.nf:
            lo_ = d[c.rank] / thr
            assert lo_ <= 1 / MARGIN, (c.seed, c.shape, lo_)
            below[kind] = max(below.get(kind, 0.0), lo_)
    for kind in sorted(above):
        print(f"rank margins rtol {kind[0]} {kind[1]}: |R_rr| >= {above[kind]:.3g} thr, |R_r+1,r+1| <= {below.get(kind, 0.0):.3g} thr")
    assert len(above) == 4
