"""Hard cases of opLDL(M, pivot=True), shared by test_ldl_pivot_hard_host.py (CPU), test_gpu_ldl_pivot_hard.py and
test_gpu_ldl_pivot_fuzz.py (-m gpu): a rational model of the Bunch-Kaufman strategy, five families of matrices whose
factorisation is exact in Float32, and a seeded generator of random cases. Plain NumPy; no device call.

The rational model. `bk_exact(M)` is ldl_pivot_cases.bunch_kaufman in fractions.Fraction: sytf2's four-way decision, the first
index on a tie, alpha the Float64 value both the device and the NumPy model use. It also counts which decision each step took,
the interchanges, the steps whose column maximum is attained more than once, and how close the closest comparison came to
equality (`margin`), so that the host test can show that no decision of the exact families hangs on a rounding of alpha.

The exact families. Every entry of L, d and e is dyadic with at most 8 significant bits, so the device has to return them bit
for bit in both precisions; every 2 x 2 block with a non-zero entry of L beneath has a zero diagonal, for which the scaled
inverse the kernel and LAPACK use is exact (t = -1).
  arrow_tie(n)            diag * I (diag = 1024) with row and column 0 set to 1 and M[0, 0] = 0. Every step but the last one is a
                          1 x 1 pivot with an interchange after a column search in which ALL remaining rows tie: the first
                          row wins, perm = 1, 2, .., n - 1, 0, and the hub's pivot ends as -(n - 1) / diag.
  gadget_sum(n, seed)     block diagonal, filled left to right by default_rng(seed) with G1 .. G4, [2] and [-4]; a gadget that
                          does not fit is replaced by [2]. G1 takes the colmax / rowmax branch and then a 2 x 2, G2 a tie and
                          1 x 1 pivots with interchanges, G3 a 2 x 2 without an interchange, G4 a 2 x 2 with an interchange and a
                          non-zero row beneath. pin = (g, col) places gadget g at column col: the panel end and the 64 / 65
                          decision meet every branch.
  saddle_pairs(n, lead)   `lead` 1 x 1 pivots +-8, q = (n - lead + 2) // 3 pairs [[0, 4], [4, 0]], t = n - lead - 2 q <= q rows with
                          diagonal 8, row j coupled to pair j only by (a, b) from {-2, -1, 1, 2}: 2 x 2 pivots without an
                          interchange and a non-zero L beneath; the trailing update must give exact zeros off the diagonal and
                          8 - a b / 2 on it. lead = 1 puts a 2 x 2 block across 63|64 (n >= 129) and 127|128 (n = 259).
  perm_blocks(n, seed)    a symmetric random permutation of a block diagonal of +-2^k, [[0, s], [s, 0]] and [[s/2, s], [s, -s/2]],
                          s = 2^k, k in -2 .. 2: L is the identity, the whole test is the interchange bookkeeping.
  bordered(n, seed)       gadget_sum(n - 1, seed) behind one 1 x 1 pivot that couples every row: L[:, 0] = 1/4, 1/2, 1/4, .. is a column
                          left of every later interchange, so the exchange of rows in the panel's finished columns and the
                          deferred pass over the columns left of a panel are compared bit for bit. Pinned so that a 65-wide
                          panel that is not the first one ends in a 2 x 2 pivot with an interchange (BORDERED_PINS).
Sizes: 2, 3, 5, 63, 64, 65, 66, 129, 130, 259 (bordered: 5, 65, 130, 259).

The fuzz generator. `case(seed)` is a function of default_rng(91000 + seed) alone, every draw made for every seed in a fixed
order, nothing rejected, in the style (and with the storage helpers) of linalg_fuzz_cases:
  family    indef, saddle0, pairs1 (ldl_pivot_cases.problem) or arrow_tie, gadget_sum, saddle_pairs, perm_blocks; the first 18 seeds force
            n = 128, 192, 256 for the three Gaussian families in both precisions
  dtype     Float64 for even seeds, Float32 for odd ones
  size      linalg_fuzz_cases.draw_size
  storage   col, row, offset (read in place), strided (copied by the constructor); NaN wherever the matrix is not
  operand   a vector, or a block of k = 2 .. 17 columns (one in eight: 24), ldv and ldr = n + 0 .. 3 independently, element
            offsets 0 .. 3, guard zones of 64 elements
  wrapper, scalars, alias   as linalg_fuzz_cases; no refine (refine > 0 with pivot=True is a ValueError)
MXLO_LDLPFUZZ_SEEDS extends the list of seeds beyond the default 160."""
import functools
import os
import types
from fractions import Fraction

import numpy as np

import ldl_pivot_cases as pc
import linalg_fuzz_cases as fz

NS = [2, 3, 5, 63, 64, 65, 66, 129, 130, 259]
ALPHA = Fraction(float(pc.ALPHA))                # the Float64 value, exactly
FAMILIES = ("arrow_tie", "gadget_sum", "saddle_pairs", "perm_blocks")           # the ones the fuzz generator draws from

G1 = [[1, 2, 0], [2, 0, 8], [0, 8, 0]]
G2 = [[0, 1, 1], [1, 2, 0], [1, 0, 2]]
G3 = [[1, 2], [2, 1]]
G4 = [[0, 0, 2], [0, 4, 1], [2, 1, 0]]
GADGETS = (G1, G2, G3, G4, [[2]], [[-4]])
PIN_COLS = (62, 63, 64)
PIN_N = 130
BORDERED_NS = (5, 65, 130, 259)
# (n, seed, (gadget, column of T)): G4 at column 63 of the matrix (panel 0 is 65 wide and ends in its interchange); G4 at column 127
# behind a 64-wide panel 0 (panel 1 is 65 wide: the interchange of its 65th column is the last one of the deferred pass); with
# seed 2 panel 2 is another one
BORDERED_PINS = ((130, 1, (4, 62)), (259, 1, (4, 126)), (259, 2, (4, 126)))


# ------------------------------------------------------------------------------------------------ the exact families
def arrow_tie(n, diag=1024.0):
    M = diag * np.eye(n)
    M[0, :] = M[:, 0] = 1.0
    M[0, 0] = 0.0
    return M


def gadget_layout(n, seed, pin=None):
    """[(first column, index into GADGETS)] of gadget_sum(n, seed, pin)"""
    rng = np.random.default_rng(seed)
    out, pos = [], 0
    while pos < n:
        limit = pin[1] if pin is not None and pos < pin[1] else n
        g = int(rng.integers(len(GADGETS)))
        if pin is not None and pos == pin[1]:
            g = pin[0] - 1
            assert pos + len(GADGETS[g]) <= n
        elif pos + len(GADGETS[g]) > limit:
            g = 4
        out.append((pos, g))
        pos += len(GADGETS[g])
    return out


def gadget_sum(n, seed, pin=None):
    M = np.zeros((n, n))
    for pos, g in gadget_layout(n, seed, pin):
        G = np.array(GADGETS[g], dtype=np.float64)
        M[pos:pos + len(G), pos:pos + len(G)] = G
    return M


def saddle_pairs(n, lead):
    assert n >= 5 and lead in (0, 1)
    rng = np.random.default_rng(4100 + 2 * n + lead)
    q = (n - lead + 2) // 3
    t = n - lead - 2 * q
    assert 0 <= t <= q
    M = np.zeros((n, n))
    for i in range(lead):
        M[i, i] = 8.0 if rng.integers(2) else -8.0
    for j in range(q):
        k = lead + 2 * j
        M[k, k + 1] = M[k + 1, k] = 4.0
    ab = rng.choice([-2.0, -1.0, 1.0, 2.0], size=(max(t, 1), 2))
    for j in range(t):
        r, k = lead + 2 * q + j, lead + 2 * j
        M[r, r] = 8.0
        M[r, k] = M[k, r] = ab[j, 0]
        M[r, k + 1] = M[k + 1, r] = ab[j, 1]
    return M


def bordered(n, seed, pin=None):
    """[[4, c'], [c, T + c c' / 4]] with T = gadget_sum(n - 1, seed, pin) and c = 1, 2, 1, 2, ..: step 0 takes the diagonal, leaves T
    exactly and L[:, 0] = c / 4, a column left of every later step whose neighbouring rows differ, so that every interchange of T's
    factorisation shows in it: inside panel 0 through the panel's finished columns, later through the deferred pass over the left
    columns. pin is in T's numbering: gadget g starts at column pin[1] + 1 of the matrix."""
    T = gadget_sum(n - 1, seed, pin)
    c = np.where(np.arange(1, n) % 2 == 1, 1.0, 2.0)
    M = np.empty((n, n))
    M[0, 0] = 4.0
    M[1:, 0] = M[0, 1:] = c
    M[1:, 1:] = T + np.outer(c, c) / 4
    return M


def panel_widths(steps, nb=64):
    """the widths of the device's panels for a sequence of steps: a panel takes steps while fewer than nb columns are done"""
    out, j0 = [], 0
    for k, kstep, _ in steps:
        if k - j0 >= nb:
            out.append(k - j0)
            j0 = k
    return out + [steps[-1][0] + steps[-1][1] - j0]


def perm_blocks(n, seed):
    rng = np.random.default_rng(seed)
    B = np.zeros((n, n))
    pos = 0
    while pos < n:
        kind, k, neg = int(rng.integers(3)), int(rng.integers(-2, 3)), bool(rng.integers(2))
        s = 2.0 ** k
        if kind == 0 or pos + 2 > n:
            B[pos, pos] = -s if neg else s
            pos += 1
            continue
        B[pos, pos + 1] = B[pos + 1, pos] = s
        if kind == 2:
            B[pos, pos], B[pos + 1, pos + 1] = s / 2, -s / 2
        pos += 2
    p = rng.permutation(n)
    return B[np.ix_(p, p)]


def exact_cases():
    """(family, arguments) of every matrix of the exact set"""
    out = []
    for n in NS:
        out.append(("arrow_tie", (n,)))
        out.append(("gadget_sum", (n, n)))
        if n >= 5:
            out += [("saddle_pairs", (n, 0)), ("saddle_pairs", (n, 1))]
        out.append(("perm_blocks", (n, n)))
    out += [("gadget_sum", (PIN_N, 100 * g + col, (g, col))) for g in (1, 2, 3, 4) for col in PIN_COLS]
    out += [("bordered", (n, n)) for n in BORDERED_NS] + [("bordered", a) for a in BORDERED_PINS]
    return out


def case_id(family, args):
    return family + "-" + "-".join(str(a).replace(" ", "") for a in args)


@functools.lru_cache(maxsize=None)
def exact_matrix(family, args):
    """the matrix (Float64, read-only), its 2-norm and its eigenvalues"""
    M = {"arrow_tie": arrow_tie, "gadget_sum": gadget_sum, "saddle_pairs": saddle_pairs, "perm_blocks": perm_blocks,
         "bordered": bordered}[family](*args)
    assert np.array_equal(M, M.T)
    w = np.linalg.eigvalsh(M)
    M.setflags(write=False)
    w.setflags(write=False)
    return M, float(np.abs(w).max()), w


@functools.lru_cache(maxsize=None)
def exact_model(family, args):
    return bk_exact(exact_matrix(family, args)[0])


@functools.lru_cache(maxsize=None)
def exact_factor(family, args):
    """(perm, L, d, e, inertia) of the rational model, rounded to Float64 (it is representable in Float32: the host test), read-only"""
    perm, L, d, e, _, _ = exact_model(family, args)
    out = (perm, as_float(L), as_float(d), as_float(e))
    for a in out:
        a.setflags(write=False)
    return out + (inertia_of(d, e),)


@functools.lru_cache(maxsize=None)
def exact_rhs(n):
    v = np.random.default_rng(7900 + n).standard_normal(n).astype(np.float32).astype(np.float64)
    v.setflags(write=False)
    return v


# ------------------------------------------------------------------------------------------------ the rational model
def bk_exact(M):
    """Bunch-Kaufman partial pivoting in rational arithmetic: (perm, L, d, e, branches, tie_steps) with M[perm][:, perm] = L D L'.
    L, d, e are object arrays of Fraction (int 0 / 1 where nothing was computed). branches: "diag" (|a_kk| >= alpha colmax),
    "ratio" (|a_kk| >= alpha colmax (colmax / rowmax)), "imax" (the 1 x 1 pivot a_imax,imax), "two" (the 2 x 2 pivot),
    "interchanges", "two_interchanged", "margin", the smallest |lhs - rhs| / rhs over all comparisons made with alpha, and "steps",
    the list of (first column, width, row interchanged with the step's last column) of every step.
    Raises ldl_pivot_cases.ZeroPivot as the NumPy model does. The trailing matrix is kept sparse and in the original numbering;
    an interchange only renumbers."""
    M = np.asarray(M, dtype=np.float64)
    n = M.shape[0]
    if not np.isfinite(M).all():
        raise ValueError("bk_exact: finite matrices only")
    S = [dict() for _ in range(n)]
    for i, j in zip(*np.nonzero(M)):
        S[int(i)][int(j)] = Fraction(float(M[i, j]))
    p = list(range(n))                           # position -> original index
    pos = list(range(n))                         # original index -> position
    cols = []                                    # per step: (k, kstep, {original row: (l0, l1)})
    d = np.zeros(n, dtype=object)
    e = np.zeros(n, dtype=object)
    br = {"diag": 0, "ratio": 0, "imax": 0, "two": 0, "interchanges": 0, "two_interchanged": 0, "margin": None, "steps": []}
    tie_steps = 0

    def compare(lhs, rhs):
        if rhs != 0:
            m = abs(lhs - rhs) / rhs
            br["margin"] = m if br["margin"] is None else min(br["margin"], m)
        return lhs >= rhs

    def search(c, k, skip):
        """(largest |entry|, its first position, how often it occurs) of row c of the trailing matrix at positions >= k, `skip` left out"""
        best, at, times = Fraction(0), None, 0
        for j, x in S[c].items():
            q = pos[j]
            if q < k or q == skip:
                continue
            a = abs(x)
            if a > best:
                best, at, times = a, q, 1
            elif a == best:
                times += 1
                if q < at:
                    at = q
        return best, at, times

    def drop(c):
        for j in S[c]:
            if j != c:
                del S[j][c]
        S[c] = {}

    k = 0
    while k < n:
        c = p[k]
        absakk = abs(S[c].get(c, Fraction(0)))
        colmax, imax, times = search(c, k + 1, -1)
        if absakk == 0 and colmax == 0:
            raise pc.ZeroPivot(k + 1)
        tie_steps += times > 1
        kstep, kp = 1, k
        if compare(absakk, ALPHA * colmax):
            br["diag"] += 1
        else:
            ci = p[imax]
            rowmax = search(ci, k, imax)[0]
            if compare(absakk, ALPHA * colmax * (colmax / rowmax)):
                br["ratio"] += 1
            elif compare(abs(S[ci].get(ci, Fraction(0))), ALPHA * rowmax):
                br["imax"] += 1
                kp = imax
            else:
                br["two"] += 1
                kp, kstep = imax, 2
        kk = k + kstep - 1
        br["steps"].append((k, kstep, kp))
        if kp != kk:
            br["interchanges"] += 1
            br["two_interchanged"] += kstep == 2
            a, b = p[kk], p[kp]
            p[kk], p[kp] = b, a
            pos[a], pos[b] = kp, kk
        if kstep == 1:
            c = p[k]
            dk = S[c].get(c, Fraction(0))
            if dk == 0:
                raise pc.ZeroPivot(k + 1)
            w = {j: x for j, x in S[c].items() if j != c}
            drop(c)
            d[k] = dk
            lcol = {j: (x / dk,) for j, x in w.items()}
            for i, (li,) in lcol.items():
                for j, wj in w.items():
                    x = S[i].get(j, 0) - li * wj
                    if x:
                        S[i][j] = x
                    else:
                        S[i].pop(j, None)
        else:
            c0, c1 = p[k], p[k + 1]
            d0, d1, e0 = S[c0].get(c0, Fraction(0)), S[c1].get(c1, Fraction(0)), S[c0].get(c1, Fraction(0))
            det = d0 * d1 - e0 * e0
            if det == 0:
                raise pc.ZeroPivot(k + 1)
            rows = (set(S[c0]) | set(S[c1])) - {c0, c1}
            w = {j: (S[c0].get(j, Fraction(0)), S[c1].get(j, Fraction(0))) for j in rows}
            drop(c0)
            drop(c1)
            d[k], d[k + 1], e[k] = d0, d1, e0
            lcol = {j: ((a * d1 - b * e0) / det, (b * d0 - a * e0) / det) for j, (a, b) in w.items()}
            for i, (l0, l1) in lcol.items():
                for j, (a, b) in w.items():
                    x = S[i].get(j, 0) - l0 * a - l1 * b
                    if x:
                        S[i][j] = x
                    else:
                        S[i].pop(j, None)
        cols.append((k, kstep, lcol))
        k += kstep
    L = np.zeros((n, n), dtype=object)
    for i in range(n):
        L[i, i] = 1
    for k, kstep, lcol in cols:
        for j, ls in lcol.items():
            for s in range(kstep):
                if ls[s]:
                    L[pos[j], k + s] = ls[s]
    return np.array(p), L, d, e, br, int(tie_steps)


def as_float(X):
    return np.asarray(X, dtype=object).astype(np.float64)


def significant_bits(x):
    """significant bits of a dyadic rational (0 for zero); None when x is not dyadic"""
    x = Fraction(x)
    den = x.denominator
    if den & (den - 1):
        return None
    num = abs(x.numerator)
    while num and not num & 1:
        num >>= 1
    return num.bit_length()


def inertia_of(d, e):
    """(positive, negative, zero) eigenvalues of the block diagonal D in exact arithmetic"""
    posi = neg = zero = 0
    k, n = 0, len(d)
    while k < n:
        if e[k] != 0:
            assert d[k] * d[k + 1] - e[k] * e[k] < 0
            posi, neg, k = posi + 1, neg + 1, k + 2
            continue
        posi, neg, zero = posi + (d[k] > 0), neg + (d[k] < 0), zero + (d[k] == 0)
        k += 1
    return int(posi), int(neg), int(zero)


# ------------------------------------------------------------------------------------------------ the tie over the stride loop
def stride_tie_n(threads):
    """the size of the arrow whose first column search gives every panel thread more than one row"""
    return 1100 if threads == 1024 else threads + 65


STRIDE_TIE_DIAG = 2.0 ** 20                      # the hub's pivot k / diag stays below alpha for every k < n


# ------------------------------------------------------------------------------------------------ the fuzz generator
BASE_SEED = 91000
DEFAULT_SEEDS = 160
FUZZ_FAMILIES = pc.CASES + FAMILIES
FORCED = [(f, n) for n in (128, 192, 256) for f in pc.CASES]         # each once per precision: seeds 2 i and 2 i + 1


def seeds():
    """the seeds of a run: 0 .. MXLO_LDLPFUZZ_SEEDS - 1, so a larger value only extends the list"""
    return range(int(os.environ.get("MXLO_LDLPFUZZ_SEEDS", str(DEFAULT_SEEDS))))


def exact_args(family, n, lead):
    return {"arrow_tie": (n,), "gadget_sum": (n, n), "saddle_pairs": (n, lead), "perm_blocks": (n, n)}[family]


def case(seed):
    rng = np.random.default_rng(BASE_SEED + seed)
    npd = np.float64 if seed % 2 == 0 else np.float32
    c = types.SimpleNamespace(seed=seed, npd=npd, eps=float(np.finfo(npd).eps), forced=seed < 2 * len(FORCED))
    # ---- every draw, in a fixed order
    family = FUZZ_FAMILIES[int(rng.integers(len(FUZZ_FAMILIES)))]
    n = fz.draw_size(rng)
    lead = int(rng.integers(2))
    storage = fz.STORAGES[int(rng.integers(4))]
    pad, off, offset_rowmajor = int(rng.integers(0, 4)), int(rng.integers(1, 4)), bool(rng.integers(2))
    vector = rng.integers(2) == 0
    k = int(rng.integers(2, 18))
    if rng.integers(8) == 0:
        k = 24
    padv, padr, offv, offr = (int(x) for x in rng.integers(0, 4, size=4))
    c.wrapper = fz.WRAPPERS[int(rng.integers(3))]
    c.scalars_index = int(rng.integers(len(fz.SCALARS)))
    alias = rng.integers(4) == 0
    # ---- family and matrix
    if c.forced:
        family, n = FORCED[seed // 2]
    c.family, c.n, c.shape = family, n, n
    c.exact = family in FAMILIES
    if c.exact:
        c.args = exact_args(family, n, lead)
        c.F, c.norm, c.eig = exact_matrix(family, c.args)
    else:
        c.args = None
        c.F, _, c.norm, c.eig = pc.problem(family, n, npd)
    c.A = c.F
    c.mf = c.nf = n
    # a factorisation with backward error 3 n eps |M| has the inertia of M as long as no eigenvalue is that close to zero; the
    # inertia is asserted where the smallest one keeps a factor 1000 from it, as test_ldl_pivot_host.py asks of the pinned cases
    c.inertia_checked = bool(np.abs(c.eig).min() >= 1000 * 3 * n * c.eps * c.norm)
    # ---- storage of the matrix
    c.storage = storage
    c.rowmajor = offset_rowmajor if storage == "offset" else storage == "row"
    c.pad, c.off = pad, (off if storage == "offset" else 0)
    # ---- the apply
    c.k = 1 if vector else k
    c.vector = bool(vector)
    c.rows_in = c.rows_out = n
    c.ldv, c.ldr, c.offv, c.offr = n + padv, n + padr, offv, offr
    c.scalars = fz.SCALARS[c.scalars_index]
    c.alias = bool(alias)
    c.V = fz.rounded(rng.standard_normal((n, c.k)), npd)
    c.res0 = fz.rounded(rng.standard_normal((n, c.k)), npd)
    if c.scalars_index == fz.NAN_RES:
        c.res0 = np.full_like(c.res0, np.nan)
    return c


def worst_eta(c, X):
    """the largest eta / (3 n eps(T)) over the columns of the result X of the plain apply to c.V"""
    return max(pc.eta(c.F, c.norm, X[:, j], c.V[:, j]) for j in range(c.k)) / (3 * c.n * c.eps)
