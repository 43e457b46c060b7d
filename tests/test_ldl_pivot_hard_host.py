"""CPU: the references and the cases of tests/ldl_pivot_hard_cases.py, which test_gpu_ldl_pivot_hard.py and
test_gpu_ldl_pivot_fuzz.py hold the device to. No device call anywhere in this file.

What is shown for every exact case: the rational factors are representable in Float32 (the bit-for-bit comparison on the device
is therefore legitimate in both precisions); a 2 x 2 block with a non-zero L beneath has a zero diagonal; the rational model,
the Float64 NumPy model and LAPACK (torch's CPU ldl_factor) agree on the permutation and the 2 x 2 positions; no comparison
with alpha comes closer than 5 % to equality, so no decision depends on how alpha times a number is rounded. Over the set every
branch occurs with and without an interchange, each gadget starts at the columns 62, 63 and 64, and a 2 x 2 block starts at
columns 63 and 127. LAPACK in the case's precision stays within 0.5 of 3 n eps on every exact case and on every fuzz seed
(measured: at most 0.048 on the exact families, 0.039 over the 160 default seeds); the coverage of the default seeds is counted."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import ldl_pivot_cases as pc
import ldl_pivot_hard_cases as hc
import test_linalg_fuzz_host as fzh

EXACT = hc.exact_cases()
IDS = [hc.case_id(*x) for x in EXACT]
HALF = 0.5
TORCH = {np.float64: torch.float64, np.float32: torch.float32}


# ------------------------------------------------------------------------------------------------ 1. the rational model
def test_the_rational_model_is_the_numpy_model_on_gaussian_matrices():
    for case, n in (("indef", 65), ("pairs1", 65), ("saddle0", 63)):
        M = pc.problem(case, n, np.float64)[0]
        perm, L, d, e, br, ties = hc.bk_exact(M)
        mperm, mL, md, me = pc.bunch_kaufman(M)
        assert np.array_equal(perm, mperm) and np.array_equal(hc.as_float(e) != 0, me != 0)
        assert np.allclose(hc.as_float(L), mL, rtol=1e-9, atol=1e-11) and np.allclose(hc.as_float(d), md, rtol=1e-9, atol=1e-11)
        assert ties == 0 and br["diag"] + br["ratio"] + br["imax"] + 2 * br["two"] == n


def test_the_rational_model_raises_as_the_numpy_model():
    for M, info in ((np.zeros((3, 3)), 1), (np.diag([1.0, 0.0, 1.0]), 2), (np.array([[1.0, 1.0], [1.0, 1.0]]), 2)):
        for model in (hc.bk_exact, pc.bunch_kaufman):
            with pytest.raises(pc.ZeroPivot) as z:
                model(M)
            assert z.value.info == info


def test_the_gadgets_take_the_branches_they_are_named_for():
    want = {0: dict(ratio=1, two=1, interchanges=0), 1: dict(imax=2, interchanges=2), 2: dict(two=1, interchanges=0),
            3: dict(two=1, two_interchanged=1, interchanges=1)}
    for g, counts in want.items():
        perm, L, d, e, br, ties = hc.bk_exact(np.array(hc.GADGETS[g], dtype=np.float64))
        for key, x in counts.items():
            assert br[key] == x, (g, key, br)
    assert hc.bk_exact(np.array(hc.G2, dtype=np.float64))[5] == 1
    L = hc.bk_exact(np.array(hc.G4, dtype=np.float64))[1]
    assert L[2, 0] != 0 or L[2, 1] != 0                    # a non-zero row beneath G4's 2 x 2 block


# ------------------------------------------------------------------------------------------------ 2. every exact case
@pytest.mark.parametrize("family,args", EXACT, ids=IDS)
def test_an_exact_case_is_representable_and_all_three_references_agree(family, args):
    M = hc.exact_matrix(family, args)[0]
    n = M.shape[0]
    assert np.array_equal(M.astype(np.float32).astype(np.float64), M)
    perm, L, d, e, br, ties = hc.exact_model(family, args)
    assert sorted(perm.tolist()) == list(range(n))
    # representable in Float32: dyadic with at most 24 significant bits (these have at most 8)
    for x in list(d) + list(e) + [L[i, j] for i, j in zip(*np.nonzero(L))]:
        b = hc.significant_bits(x)
        assert b is not None and b <= 8, (family, args, x)
        assert x == 0 or Fraction(2) ** -100 <= abs(x) <= Fraction(2) ** 100
    # the factors reconstruct the permuted matrix exactly
    Lf, df, ef = hc.as_float(L), hc.as_float(d), hc.as_float(e)
    assert np.array_equal(Lf @ pc.block_diag_of(df, ef) @ Lf.T, M[np.ix_(perm, perm)])
    # a 2 x 2 block with a non-zero L beneath has a zero diagonal
    two = [k for k in range(n) if e[k] != 0]
    for k in two:
        assert e[k + 1] == 0 and L[k + 1, k] == 0
        if np.any(Lf[k + 2:, k:k + 2]):
            assert d[k] == 0 and d[k + 1] == 0, (family, args, k)
    # the NumPy model and LAPACK take the same pivots
    mperm, _, _, me = pc.bunch_kaufman(M)
    assert np.array_equal(perm, mperm) and set(np.nonzero(me)[0].tolist()) == set(two)
    lperm, ltwo = pc.lapack_pivots(M)
    assert np.array_equal(perm, lperm) and ltwo == set(two)
    # no decision hangs on a rounding
    assert br["margin"] is None or br["margin"] >= Fraction(1, 20), (family, args, float(br["margin"]))
    assert hc.inertia_of(d, e) == (int((hc.exact_matrix(family, args)[2] > 0).sum()), int((hc.exact_matrix(family, args)[2] < 0).sum()), 0)
    if family == "arrow_tie":
        assert ties == max(n - 2, 0) and br["imax"] == br["interchanges"] == n - 1
        assert np.array_equal(perm, np.r_[1:n, 0]) and d[n - 1] == Fraction(-(n - 1), 1024)
    if family == "saddle_pairs":
        q = (n - args[1] + 2) // 3
        assert br["two"] == q and br["interchanges"] == 0 and np.count_nonzero(Lf - np.eye(n)) == 2 * (n - args[1] - 2 * q)
    if family == "perm_blocks":
        assert np.array_equal(Lf, np.eye(n))


def test_the_exact_set_covers_every_branch_panel_end_and_gadget_position():
    total = {}
    starts = {g: set() for g in range(4)}
    two_at = set()
    for family, args in EXACT:
        perm, L, d, e, br, ties = hc.exact_model(family, args)
        n = len(d)
        for key, x in br.items():
            if key not in ("margin", "steps"):
                total[key] = total.get(key, 0) + x
        total["two_in_place"] = total.get("two_in_place", 0) + br["two"] - br["two_interchanged"]
        total["one_interchanged"] = total.get("one_interchanged", 0) + br["interchanges"] - br["two_interchanged"]
        two_at |= {k for k in range(n) if e[k] != 0}
        if family == "gadget_sum":
            for pos, g in hc.gadget_layout(*args):
                if g < 4:
                    starts[g].add(pos)
    print("branches over the exact set:", total)
    for key in ("diag", "ratio", "imax", "two", "two_interchanged", "two_in_place", "one_interchanged"):
        assert total[key] >= 10, (key, total)
    for g in range(4):
        assert set(hc.PIN_COLS) <= starts[g], (g, sorted(starts[g]))
    assert 63 in two_at and 127 in two_at
    # a 65-wide panel behind the first one whose last step is a 2 x 2 pivot with an interchange of two rows that differ in a
    # column left of the panel: the last interchange of the deferred pass over the left columns
    late = 0
    for family, args in EXACT:
        if family != "bordered":
            continue
        perm, L, d, e, br, ties = hc.exact_model(family, args)
        widths = hc.panel_widths(br["steps"])
        assert sum(widths) == len(d) and all(w in (64, 65) for w in widths[:-1]) and 1 <= widths[-1] <= 65
        begins = np.cumsum([0] + widths)
        for r, w in enumerate(widths):
            if w == 65:
                k, kstep, kp = next(s for s in br["steps"] if s[0] == begins[r] + 63)
                assert kstep == 2
                if r >= 1 and kp != k + 1 and L[k + 1, 0] != L[kp, 0]:
                    late += 1
    assert late >= 3
    for n in (63, 64, 65, 66, 129, 130, 259):               # with seed = n every branch occurs in one matrix
        br = hc.exact_model("gadget_sum", (n, n))[4]
        assert br["ratio"] and br["imax"] and br["two"] > br["two_interchanged"] > 0 and br["diag"], (n, br)


def test_the_stride_tie_case_keeps_the_hub_below_alpha():
    n = hc.stride_tie_n(1024)
    assert n == 1100 and hc.stride_tie_n(256) == 321
    assert (n - 1) / hc.STRIDE_TIE_DIAG < 0.05 * pc.ALPHA and (n - 1) / 1024.0 > pc.ALPHA      # 1024 would not do at this size
    for m in (n, hc.stride_tie_n(256)):
        perm, L, d, e, br, ties = hc.exact_model("arrow_tie", (m, hc.STRIDE_TIE_DIAG))
        assert np.array_equal(perm, np.r_[1:m, 0]) and ties == m - 2 and br["imax"] == m - 1 and not any(e)
        assert d[m - 1] == Fraction(-(m - 1), 2 ** 20) and all(x == 2 ** 20 for x in d[:m - 1])


# ------------------------------------------------------------------------------------------------ 3. LAPACK against the bound
def lapack_fraction(M, nM, V, npd):
    """the worst eta / (3 n eps) of sytrf / sytrs in the precision npd over the columns of V"""
    n = M.shape[0]
    worst = 0.0
    for j in range(V.shape[1]):
        x = pc.lapack_solve(M, V[:, j], TORCH[npd])
        assert np.isfinite(x).all()
        worst = max(worst, pc.eta(M, nM, x, V[:, j]) / (3 * n * float(np.finfo(npd).eps)))
    return worst


def test_lapack_stays_within_half_of_the_bound_on_the_exact_families():
    worst = 0.0
    for family, args in EXACT:
        M, nM, _ = hc.exact_matrix(family, args)
        for npd in (np.float64, np.float32):
            r = lapack_fraction(M, nM, hc.exact_rhs(M.shape[0])[:, None], npd)
            worst = max(worst, r)
            assert r <= HALF, (family, args, npd.__name__, r)
    print(f"LAPACK on the exact families: at most {worst:.4f} of 3 n eps")


@pytest.fixture(scope="module")
def cases():
    return [hc.case(s) for s in hc.seeds()]


def test_lapack_stays_within_half_of_the_bound_on_every_fuzz_seed(cases):
    worst = {}
    for c in cases:
        r = lapack_fraction(c.F, c.norm, c.V, c.npd)
        worst[c.family] = max(worst.get(c.family, 0.0), r)
        assert r <= HALF, (c.seed, c.family, c.n, c.npd.__name__, r)
    for f in sorted(worst):
        print(f"LAPACK / (3 n eps) {f}: {worst[f]:.4f}")
    assert set(worst) == set(hc.FUZZ_FAMILIES)


# ------------------------------------------------------------------------------------------------ 4. the fuzz generator
def test_a_fuzz_case_is_a_function_of_its_seed_and_the_variable_only_extends_the_list(cases, monkeypatch):
    for c in cases[:40]:
        assert fzh.equal_cases(c, hc.case(c.seed)), c.seed
    monkeypatch.delenv("MXLO_LDLPFUZZ_SEEDS", raising=False)
    default = list(hc.seeds())
    assert default == list(range(hc.DEFAULT_SEEDS)) and hc.DEFAULT_SEEDS >= 2 * len(hc.FORCED)
    monkeypatch.setenv("MXLO_LDLPFUZZ_SEEDS", str(hc.DEFAULT_SEEDS + 5))
    assert list(hc.seeds()) == default + list(range(hc.DEFAULT_SEEDS, hc.DEFAULT_SEEDS + 5))


def test_the_fuzz_storage_puts_the_matrix_where_it_says(cases):
    import linalg_fuzz_cases as fz
    for c in cases:
        buf, shape, strides, offset = fz.matrix_storage(c)
        assert buf.dtype == c.npd and shape == (c.n, c.n)
        assert np.array_equal(fz.window(buf, shape, strides, offset), c.F)
        assert np.isnan(fz.outside(buf, shape, strides, offset).view(c.npd)).all()
        assert np.array_equal(c.F.astype(c.npd).astype(np.float64), c.F)


def test_the_default_fuzz_seeds_reach_what_they_are_meant_to_reach():
    """Minimum counts over the 160 default seeds, chosen from what the generator yields (printed): every family 12 times and 4
    times per precision, every storage 25, every wrapper 40, every scalar form 20, vectors and blocks 60 each, ragged groups 40,
    full groups 8, k = 17 and k = 24 at least once, ldr != ldv 30, alias 25, an operand off the 16-byte phase 60; the inertia is
    asserted at least twice per family and precision (Float32: indef 3 times, saddle0 twice; every Float64 case)."""
    cs = [hc.case(s) for s in range(hc.DEFAULT_SEEDS)]
    counts = {}

    def count(*key):
        counts[key] = counts.get(key, 0) + 1

    for c in cs:
        count("family", c.family)
        count("family", c.family, c.npd.__name__)
        count("storage", c.storage)
        count("wrapper", c.wrapper)
        count("scalars", c.scalars_index)
        count("operand", "vector" if c.vector else "block")
        if not c.vector:
            count("group", "ragged" if c.k % 8 else "full")
            count("k", c.k)
            if c.ldr != c.ldv:
                count("ldr != ldv")
        if c.alias:
            count("alias")
        if c.inertia_checked or c.exact:
            count("inertia", c.family, c.npd.__name__)
        if (c.offv * c.F.itemsize) % 16 or (c.offr * c.F.itemsize) % 16:
            count("off phase")
    for key in sorted(counts, key=str):
        print(f"coverage {key}: {counts[key]}")
    want = ([(("family", f), 12) for f in hc.FUZZ_FAMILIES]
            + [(("family", f, p), 4) for f in hc.FUZZ_FAMILIES for p in ("float64", "float32")]
            + [(("inertia", f, p), 2) for f in hc.FUZZ_FAMILIES for p in ("float64", "float32")]
            + [(("storage", s), 25) for s in ("col", "row", "offset", "strided")]
            + [(("wrapper", w), 40) for w in ("op", "transpose", "adjoint")] + [(("scalars", i), 20) for i in range(5)]
            + [(("operand", "vector"), 60), (("operand", "block"), 60), (("group", "ragged"), 40), (("group", "full"), 8),
               (("k", 17), 1), (("k", 24), 1), (("ldr != ldv",), 30), (("alias",), 25), (("off phase",), 60)])
    short = {key: counts.get(key, 0) for key, least in want if counts.get(key, 0) < least}
    assert not short, short
    for family, n in hc.FORCED:
        for npd in (np.float64, np.float32):
            assert sum(c.forced for c in cs if c.family == family and c.n == n and c.npd is npd) == 1, (family, n)
    assert all(8 <= c.n <= 259 for c in cs)
