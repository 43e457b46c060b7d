"""The table behind test_forms_host.py (CPU) and test_gpu_forms.py (device): for every tuning key of a ctx
(csrc/tune_keys.def) the values to set, the operator family that consumes the key and the small, ragged, misaligned shapes
to run it on — or the reason why no parity test can exist. Plain data and seeded NumPy inputs; nothing here touches a GPU.

Contract under test: every value mxlo_ctx_tune accepts gives the operator's correct result on every shape the operator
accepts. A key that csrc/tune_keys.def gains fails test_forms_host.py until it has a row in FORMS or a reason in EXCLUDED.

A row is a dict:
  values    the values of the key to run (lowest, highest, every listed value; for a threshold one value on each side of
            the footprint of the row's shapes). HI_PER_CU stands for highest // (number of CUs), the largest value the setter
            takes for `red_blocks_per_cu` on the device at hand.
  family    name of the runner in test_gpu_forms.py (RUNNERS): it builds the operands from `shapes`, applies the operator
            (3-argument form and (alpha, beta) = (2, -3)), compares with the family's oracle at the family's own tolerance
            and returns every output.
  shapes    what the runner iterates over (never empty).
  fixed     other keys held while the row runs — for the tested value AND for the default-form result it is compared with.
  bitwise   True: every output must have the bits of the default-form result (key at its enumerated default, `fixed`
            applied). Decided by reading the kernel: `why` says why in one line, `at` is the file:line it rests on.
            False: the two results are compared at the tolerance of tests/test_gpu_qn.py:871 (1e-12 / 2e-5 relative L2).
            These norms are parity with the oracle, not the accumulation contract: tests/f32_contract_cases.py and
            tests/test_gpu_f32_contract.py hold the Float32 / ComplexF32 reductions of the dots, Householder, dense, Hermitian,
            sparse and block-diagonal families, under the same keys and shapes, to Float64 accumulation per element, to the bit.
  engaged   {value: kernel launches of one apply} at the row's `probe` shape (mxlo_debug_counters()[10]); for the dense family
            a pair: the launches of M v and of M V.
"""
import functools

import numpy as np

HI_PER_CU = "highest // num_cu"
I64_MAX = (1 << 63) - 1
MIB = 1 << 20
BETWEEN_FORMS = {8: 1e-12, 4: 2e-5}                  # tests/test_gpu_qn.py:871, by bytes of the real element type

# element types by name (the runners map them to torch / numpy types); V = 16 / element size
V = {"f64": 2, "f32": 4, "c128": 1}
# the five forms that may refuse at run time on a shared card (co-residency query, XCD probe): assertion 3 is waived for them
WAIVABLE = ("house_fused", "qn_fused_small", "qn_persist", "herm_single", "kron_fuse")


def stream_sizes(t):
    v = V[t]
    return [1, 4 * v - 1, 4 * v, 1023, 1025, 65_537]


def red_sizes(t):
    v = V[t]
    return [4 * v - 1, 4 * v, 4099, 300_001]


def row(values, family, shapes, bitwise=False, why=None, at=None, fixed=None, engaged=None, probe=None):
    return dict(values=list(values), family=family, shapes=shapes, bitwise=bitwise, why=why, at=at, fixed=dict(fixed or {}),
                engaged=engaged, probe=probe)


# ------------------------------------------------------------------------------------------------ shapes of the families
STREAM = [(t, n) for t in ("f64", "f32", "c128") for n in stream_sizes(t)]
# (element size, nres): the sorted extension works on 16 KiB tiles of 4-, 8- and 16-byte elements (leaves.hip:785)
EXTEND = [(es, nres) for es in (4, 8, 16) for tile in (16384 // es,) for nres in (tile - 1, tile, tile + 1, 3 * tile + 1, 40 * tile + 5)]
DOTS = [(t, n) for t in ("f64", "f32", "c128") for n in red_sizes(t) + [1 << 20]]
HOUSE = [(t, n) for t in ("f64", "f32") for n in red_sizes(t)]
# (kind, element type, mem, pairs pushed, n): 2, 4, 5, 21 and 40 panel columns when the memory is full; every n of red_sizes
QN4 = [("inv", "f64", 1, 3, 7), ("fwd", "f64", 2, 4, 8), ("inv", "f32", 2, 3, 15), ("fwd", "f32", 1, 3, 16), ("lsr1", "f64", 5, 7, 4099),
       ("lsr1", "f32", 21, 23, 4099), ("inv", "f64", 20, 22, 4099), ("fwd", "f32", 20, 22, 4099), ("lsr1", "f64", 5, 3, 300_001),
       ("inv", "f64", 5, 7, 300_001), ("fwd", "f64", 2, 3, 300_001)]
KRYLOV = [("f64", 257, 5), ("f32", 257, 5), ("f64", 4099, 33), ("f32", 4099, 33)]
DIAGQN = [(t, kind, n) for t in ("f32", "f64") for kind in ("psb", "andrei", "bfgs", "spectral") for n in red_sizes(t)]
# single-launch apply: <= 12 columns (mem 5: 10) and > 12 (mem 10: 20, LSR1 mem 20: 20); n = 7 keeps the memory below n
QNF = [("inv", "f64", 3, 7), ("fwd", "f64", 3, 7)] + [(kind, "f64", mem, n) for n in (4099, 65_536, 65_537, 131_071)
                                                       for kind, mem in (("inv", 5), ("fwd", 10), ("lsr1", 20))] + \
      [("inv", "f32", 5, 65_537), ("lsr1", "f32", 5, 131_071)]
QNP = [("inv", "f64", 1, 4099), ("lsr1", "f64", 5, 4099), ("fwd", "f64", 20, 4099), ("inv", "f64", 5, 65_537), ("fwd", "f32", 5, 65_537),
       ("lsr1", "f64", 20, 65_537), ("inv", "f64", 5, (1 << 19) + 5), ("lsr1", "f32", 1, (1 << 19) + 5)]
INVMODE = [("f64", 3, 7), ("f64", 5, 4099), ("f32", 5, 4099), ("f64", 20, 4099)]
# (SR1 on n = 4V - 1 with 5 pairs is rounding noise in the reference too: the L-BFGS kinds take the short vectors)
PUSH = [(kind, t, mem, n) for kind in ("inv", "fwd", "lsr1") for t, mem, n in (("f64", 5, 7), ("f64", 20, 4099), ("f32", 25, 4099),
                                                                            ("f64", 40, 4099), ("f32", 5, 15), ("f64", 5, 4099))
        if not (kind == "lsr1" and n < 100)]
# (kind, element type, mem, n, (phase of s, phase of y)): a pair whose vectors start at DIFFERENT 16-byte phases leaves the one-pass
# push (qn.hip:2299, 2605); the decision dots are then panel_dots over the caller's own vectors — {s, y} (qn.hip:2304) or
# {y, s, y - B s} (qn.hip:2623) — whose columns are mixed-phase: the scalar fallback of reductions.hip:298-304 on several workgroups
PUSHMIX = [(kind, t, 5, n, ph) for kind in ("inv", "fwd", "lsr1") for t, n, ph in (("f64", 4099, (0, 1)), ("f32", 4099, (1, 2)),
                                                                                ("f64", 300_001, (1, 0)), ("f32", 300_001, (0, 3)))]
# (element type, m, n, extra leading dimension): f32 takes twice the m, so both cross the m >= 4 * 128 * V gate of dense.hip:1032
# (1030 and 2052 rows: a multiple of V that is no multiple of a row band of 8 V, 16 V or 32 V rows — a ragged last band)
# The last two: the smallest shapes at which `auto` takes the row bands by itself on 256 CUs — n >= 1024 and m >= 8 V x CUs
# (dense.hip:392-397, 977-980) — with m no multiple of the band of 8 V rows: a ragged last band (33 MB each).
GEMV = [("f64", 1024, 33, 0), ("f64", 1025, 31, 1), ("f64", 2049, 64, 0), ("f64", 1030, 40, 0), ("f32", 2048, 33, 0), ("f32", 2050, 31, 1),
        ("f32", 4098, 64, 0), ("f32", 2052, 40, 0), ("f64", 4098, 1024, 0), ("f32", 8196, 1024, 0)]
GEMV_BAND = GEMV[-2:]
GEMV_K = (4, 8, 9)
HERM = [(t, n) for t in ("f64", "f32", "c128") for n in (256, 512, 515)]
KRON = [("f64", (64, 64), (64, 64)), ("f64", (96, 40), (96, 40)), ("f64", (33, 17), (33, 17)), ("f32", (64, 64), (64, 64)),
        ("f32", (96, 40), (40, 96)), ("f32", (33, 17), (17, 33))]
# sparse: (element type, chunks of the N apply, one row longer than a chunk: pieces + the fix-up launch); the runner sizes the
# matrix for the count and reads it back from mxlo_csc_info. 1, 3, sp_xcds + 1 = 9 and 65 chunks.
SPARSE = [("f64", 1, False), ("f64", 3, False), ("f64", 9, True), ("f32", 65, False)]
BLOCKDIAG = ["f64", "f32"]
CGEMV = [("c128", 65, 7), ("c128", 257, 300)]


# ------------------------------------------------------------------------------------------------ the table
_NT_WHY = "NT is a template parameter that only selects the cache policy of ldg / stg"
_QN4 = dict(qn_fused_small=0, qn_persist=0)
_PERSIST = dict(qn_persist=1, qn_persist_min_n=1, qn_persist_min_bytes=0)

FORMS = {
    "blocks_per_cu": [
        row([0, 1, 64], "stream", STREAM, True, "only the grid of the grid-stride map_kernel changes: every element is still produced once by the same op",
            "linearoperators.jl_amd/csrc/stream_kernels.h:170"),
        row([0, 1, 64], "restrict", STREAM, True, "gather / scatter copy elements: the grid decides who copies, not what",
            "linearoperators.jl_amd/csrc/leaves.hip:684"),
    ],
    "nt_min_bytes": [
        row([0, I64_MAX], "stream", STREAM, True, _NT_WHY, "linearoperators.jl_amd/csrc/stream_kernels.h:166"),
        row([0], "restrict", STREAM, True, "the gather / scatter kernels have no NT instantiation and never read the key",
            "linearoperators.jl_amd/csrc/leaves.hip:686"),
        row([0], "dots", DOTS),      # reductions.hip:240: with nt on, one- and two-column dots take ONE workgroup per CU — a grid change
        row([0], "house2", HOUSE, fixed=dict(house_fused=0, house_inline_n=0)),
        row([0], "qn4", QN4, fixed=_QN4),
        row([0], "krylov", KRYLOV),
        row([0], "diagqn", DIAGQN),
        row([0], "gemv", GEMV),
        row([0], "gemv", GEMV, fixed=dict(gemv_n_rows=32)),      # an explicit band height (16 V / 8 V rows) with nontemporal loads at every shape
        row([0], "push", PUSHMIX),
        row([0], "sparse", SPARSE, True, "the sparse apply has no NT instantiation and never reads the key", "linearoperators.jl_amd/csrc/sparse.hip:121"),
        row([0], "blockdiag", BLOCKDIAG, True, _NT_WHY, "linearoperators.jl_amd/csrc/blockdiag.hip:370"),
        row([0], "cgemv", CGEMV, True, _NT_WHY, "linearoperators.jl_amd/csrc/complex.hip:456"),
    ],
    "extend_tiles_per_block": [
        row([0, 1, 1024], "extend", EXTEND, True, "tiles per workgroup: each output tile is still written once from the same plan search",
            "linearoperators.jl_amd/csrc/leaves.hip:765"),
    ],
    "red_blocks_per_cu": [
        row([1, 4, HI_PER_CU], "dots", DOTS),
        row([1, HI_PER_CU], "house2", HOUSE, fixed=dict(house_fused=0)),
        row([1, HI_PER_CU], "house2", HOUSE, fixed=dict(house_fused=0, house_inline_n=0)),
        row([1, HI_PER_CU], "qn4", QN4, fixed=_QN4),
        row([1, HI_PER_CU], "krylov", KRYLOV),
        row([1, HI_PER_CU], "diagqn", DIAGQN),
        row([1, HI_PER_CU], "push", PUSHMIX),
    ],
    "fuse_finalize": [
        row([0, 1], "dots", DOTS),
        row([0, 1], "house2", HOUSE, fixed=dict(house_fused=0, house_inline_n=0)),
        row([0, 1], "qn4", QN4, fixed=_QN4),
        row([0, 1], "push", PUSHMIX),
    ],
    # (mxlo_dot has one column and csrc/krylov.hip never reads the key: neither family has a row here)
    "dots_max_nc": [
        row([1, 3, 20], "qn4", QN4, fixed=_QN4),
        row([1, 3, 20], "push", PUSHMIX),
    ],
    "house_fused": [
        row([0, 1], "house", HOUSE, engaged={0: 2, 1: 1}, probe=("f64", 4099)),
    ],
    "house_fused_per_cu": [
        row([1, 2], "house", HOUSE + [("f64", (1 << 20) + 3)]),
    ],
    "house_reverse": [
        row([0, 1], "house2", HOUSE, True, "REVERSE is the order in which the elementwise update walks the vectors",
            "linearoperators.jl_amd/csrc/leaves.hip:373", fixed=dict(house_fused=0)),
        row([0, 1], "house2", HOUSE, True, "REVERSE is the order in which the elementwise update walks the vectors",
            "linearoperators.jl_amd/csrc/leaves.hip:226", fixed=dict(house_fused=0, house_inline_n=0)),
    ],
    "house_inline_n": [
        # fuse_finalize = 0 makes the two forms differ in launches: dots + update (inline, n <= the key) against dots + finalize + update
        row([0, 4098, 4099, 1 << 23, I64_MAX], "house2", HOUSE, fixed=dict(house_fused=0, fuse_finalize=0),
            engaged={0: 3, 4098: 3, 4099: 2, 1 << 23: 2, I64_MAX: 2}, probe=("f64", 4099)),
    ],
    "combine_blocks_per_cu": [
        row([0, 1, 64], "qn4", QN4, True, "the grid of the combine pass: every output element is the same fixed-order sum over the columns",
            "linearoperators.jl_amd/csrc/qn.hip:349", fixed=_QN4),
    ],
    "combine_reverse": [
        row([0, 1], "qn4", QN4, True, "the order in which the combine pass walks the (independent) output vectors",
            "linearoperators.jl_amd/csrc/qn.hip:1386", fixed=_QN4),
    ],
    # (the probe's n = 4099 is odd: the four-launch form takes a fifth, scalar combine launch for the last element, qn.hip:384-388)
    "qn_fused_small": [
        row([0, 1], "qnf", QNF, fixed=dict(qn_persist=0), engaged={0: 5, 1: 1}, probe=("inv", "f64", 5, 4099)),
    ],
    "qn_fused_batch12": [
        row([0, 1], "qnf", QNF, fixed=dict(qn_persist=0)),
    ],
    "qn_fused_max_grid": [
        # n = 65 536 doubles in 10 columns: 64 workgroups of two vectors per lane (qn.hip:944-951) — above 8, within 256
        row([1, 8, 256], "qnf", QNF, fixed=dict(qn_persist=0), engaged={1: 4, 8: 4, 256: 1}, probe=("inv", "f64", 5, 65_536)),
    ],
    # The four-launch form of the probe (n = 65 537 doubles, odd) is FIVE launches: dots, finalize, coefficients, the combine
    # on the whole 16-byte vectors and a second, scalar combine launch for the one element behind them (qn.hip:384-388).
    "qn_persist": [
        row([0, 1], "qnp", QNP, fixed=dict(qn_persist_min_n=1, qn_persist_min_bytes=0, qn_fused_small=0), engaged={0: 5, 1: 1},
            probe=("inv", "f64", 5, 65_537)),
    ],
    "qn_persist_min_n": [
        row([1, 65_537, 65_538, 1 << 19, I64_MAX], "qnp", QNP, fixed=dict(qn_persist_min_bytes=0, qn_fused_small=0),
            engaged={1: 1, 65_537: 1, 65_538: 5, 1 << 19: 5, I64_MAX: 5}, probe=("inv", "f64", 5, 65_537)),
    ],
    "qn_persist_min_bytes": [
        # the probe's panel: 10 columns x 65 537 doubles = 5 242 960 bytes
        row([0, 5_242_960, 5_242_961, 32 * MIB, I64_MAX], "qnp", QNP, fixed=dict(qn_persist_min_n=1, qn_fused_small=0),
            engaged={0: 1, 5_242_960: 1, 5_242_961: 5, 32 * MIB: 5, I64_MAX: 5}, probe=("inv", "f64", 5, 65_537)),
    ],
    "qn_persist_max_bytes": [
        row([0, 5_242_959, 5_242_960, 448 * MIB, I64_MAX], "qnp", QNP, fixed=dict(qn_persist_min_n=1, qn_persist_min_bytes=0, qn_fused_small=0),
            engaged={0: 5, 5_242_959: 5, 5_242_960: 1, 448 * MIB: 1, I64_MAX: 1}, probe=("inv", "f64", 5, 65_537)),
    ],
    "qn_persist_reverse": [
        row([0, 1], "qnp", QNP, True, "the order in which a workgroup's combine phase walks its own (independent) chunks",
            "linearoperators.jl_amd/csrc/qn.hip:1325", fixed=_PERSIST, engaged={0: 1, 1: 1}, probe=("inv", "f64", 5, 65_537)),
    ],
    "qn_persist_prefetch": [
        row([0, 1], "qnp", QNP, True, "loads issued earlier; values and the order of every operation stay",
            "linearoperators.jl_amd/csrc/qn.hip:1325", fixed=_PERSIST, engaged={0: 1, 1: 1}, probe=("inv", "f64", 5, 65_537)),
    ],
    "qn_persist_lds": [
        row([0, 1], "qnp", QNP, True, "the combine phase reads x and the first columns from LDS copies instead of memory: same values",
            "linearoperators.jl_amd/csrc/qn.hip:1308", fixed=_PERSIST, engaged={0: 1, 1: 1}, probe=("inv", "f64", 5, 65_537)),
    ],
    "qn_persist_lds_pad": [
        row([0, 81_920, 114_688], "qnp", QNP, True, "dynamic LDS the kernel never touches", "linearoperators.jl_amd/csrc/qn.hip:1307",
            fixed=_PERSIST, engaged={0: 1, 81_920: 1, 114_688: 1}, probe=("inv", "f64", 5, 65_537)),
    ],
    "lbfgs_inv_mode": [
        row([0, 1], "invmode", INVMODE),
    ],
    "push_fused": [
        row([0, 1], "push", PUSH),
    ],
    "push_wide": [
        row([0, 1], "push", PUSH),
    ],
    "push_posted": [
        row([0, 1], "push", PUSH, True, "the same kernels; only the way the decision scalars reach the host changes",
            "linearoperators.jl_amd/csrc/qn.hip:1568"),
    ],
    # 0 off, 1 auto; a band height is taken where it is 8 V, 16 V or 32 V rows (16 / 32 / 64 for Float64, 32 / 64 / 128 for Float32,
    # dense.hip:391) and leaves the column-chunk schedule in place otherwise (7; 128 for Float64; 16 for Float32)
    "gemv_n_rows": [
        # launches of (M v, M V) at the probe: one where the row bands run, two (partials + finish) in the column-chunk schedule
        row([0, 1, 7, 16, 32, 64, 128], "gemv", GEMV, probe=GEMV_BAND[0],
            engaged={0: (2, 1), 1: (1, 1), 7: (2, 1), 16: (1, 1), 32: (1, 1), 64: (1, 1), 128: (2, 1)}),
    ],
    "gemvb_n_rows": [
        row([0, 1], "gemv", GEMV, engaged={0: (1, 2), 1: (1, 1)}, probe=GEMV_BAND[0]),
    ],
    "gemvb_t_lds": [
        row([0, 1], "gemv", GEMV),
    ],
    "herm_nt": [
        row([-1, 0, 1], "herm", HERM, True, "NT is a template parameter of the pass kernels: the cache policy of the strip loads",
            "linearoperators.jl_amd/csrc/dense.hip:1577"),
        # (the single launch takes the real vector applies at n = 256 / 512 and has no NT instantiation: the two launches do)
        row([-1, 0, 1], "herm", HERM, True, "NT is a template parameter of the pass kernels: the cache policy of the strip loads",
            "linearoperators.jl_amd/csrc/dense.hip:1577", fixed=dict(herm_single=0)),
    ],
    # an n = 512 Float64 triangle is 8 * 512 * 256 = 1 MiB: below dp_min (nontemporal), in [dp_min, nt_min) (default policy), from nt_min on
    "herm_dp_min_bytes": [
        row([0, MIB, MIB + 1, 96 * MIB, I64_MAX], "herm", HERM, True, "selects the cache policy of the strip loads only",
            "linearoperators.jl_amd/csrc/dense.hip:1579", fixed=dict(herm_nt=-1, herm_nt_min_bytes=2 * MIB)),
        row([0, MIB, MIB + 1, 96 * MIB, I64_MAX], "herm", HERM, True, "selects the cache policy of the strip loads only",
            "linearoperators.jl_amd/csrc/dense.hip:1579", fixed=dict(herm_nt=-1, herm_nt_min_bytes=2 * MIB, herm_single=0)),
    ],
    "herm_nt_min_bytes": [
        row([0, MIB, MIB + 1, 384 * MIB, I64_MAX], "herm", HERM, True, "selects the cache policy of the strip loads only",
            "linearoperators.jl_amd/csrc/complex.hip:964", fixed=dict(herm_nt=-1, herm_dp_min_bytes=0)),
        row([0, MIB, MIB + 1, 384 * MIB, I64_MAX], "herm", HERM, True, "selects the cache policy of the strip loads only",
            "linearoperators.jl_amd/csrc/dense.hip:1579", fixed=dict(herm_nt=-1, herm_dp_min_bytes=0, herm_single=0)),
    ],
    "herm_lds_pad": [
        row([0, 49_152], "herm", HERM, True, "dynamic LDS the pass kernels never touch", "linearoperators.jl_amd/csrc/dense.hip:1687",
            fixed=dict(herm_single=0)),
    ],
    "herm_poll_sleep": [
        row([1, 4, 1024], "herm", HERM, True, "how often the finishers of the single launch look for their slots", "linearoperators.jl_amd/csrc/dense.hip:1651"),
    ],
    "herm_order": [
        row([0, 1], "herm", HERM, True, "the order of the interior strips: every partial lands in the same slot and is added in the same order",
            "linearoperators.jl_amd/csrc/dense.hip:1688"),
        row([0, 1], "herm", HERM, True, "the order of the interior strips: every partial lands in the same slot and is added in the same order",
            "linearoperators.jl_amd/csrc/dense.hip:1688", fixed=dict(herm_single=0)),
    ],
    "herm_strip": [
        row([0, 1, 2, 8], "herm", HERM),
    ],
    "cherm_two_pass": [
        row([0, 1], "herm", [s for s in HERM if s[0] == "c128"]),
    ],
    "herm_single": [
        row([0, 1], "herm", HERM, True, "strips and finishers share the partial layout and the order of the additions with the two launches",
            "linearoperators.jl_amd/csrc/dense.hip:1616", engaged={0: 2, 1: 1}, probe=("f64", 512)),
    ],
    "herm_single_max_n": [
        row([0, 511, 512, I64_MAX], "herm", HERM, engaged={0: 1, 511: 2, 512: 1, I64_MAX: 1}, probe=("f64", 512)),
    ],
    "herm_single_max_bytes": [
        row([0, MIB - 1, MIB, 112 * MIB, I64_MAX], "herm", HERM, engaged={0: 2, MIB - 1: 2, MIB: 1, 112 * MIB: 1, I64_MAX: 1}, probe=("f64", 512)),
    ],
    "gemm_tile": [
        row([-1, 0, 32, 64, 128], "kron", KRON, fixed=dict(kron_fuse=0)),
    ],
    "kron_fuse": [
        row([0, 1], "kron", KRON, engaged={0: 2, 1: 1}, probe=("f64", (64, 64), (64, 64))),
    ],
    "sp_xcds": [
        row([1, 8, 64], "sparse", SPARSE, True, "a permutation of the chunk -> workgroup map; workgroups past the last chunk return",
            "linearoperators.jl_amd/csrc/sparse.hip:54"),
    ],
}

EXCLUDED = {
    "fused_timeout_ms": "no second form: how long a single-launch workgroup polls. tests/test_gpu_leaves.py::test_single_launch_householder_timeout_is_an_error_not_a_hang "
                        "and tests/test_gpu_qn.py::test_single_launch_apply_timeout_is_an_error_not_a_hang set and time it; shortening it here could only make a form refuse",
    "fused_debug_drop": "test hook that makes a workgroup withhold its partial (NaN result by design); covered by the three *_timeout_is_an_error_not_a_hang tests",
    "alias_guard": "test hook: 0 hands overlapping operands to racing kernels, wrong results by design (csrc/common.h: stage_alias); "
                   "the guarded value is what tests/test_gpu_aliasing.py runs",
    "graph_direct_max": "replay policy of captured chains (direct launches or hipGraphLaunch), not a kernel form; "
                        "tests/test_gpu_contract.py replays captured applies on both sides of it",
}
# single values left out of a key that has rows
EXCLUDED_VALUES = {
    ("kron_fuse", 2): "timing experiment without the wait: wrong results by design (tests/test_gpu_tune.py::test_leaving_the_no_wait_kron_mode_through_tuned_rearms_the_counters)",
    ("push_posted", 2): "debug hook that treats every posting as lost; tests/test_gpu_qn.py::test_posted_read_back_of_the_push_decision runs it",
}
LISTS = {"gemm_tile": (-1, 0, 32, 64, 128), "herm_strip": (0, 1, 2, 8)}


def cases():
    """(key, row index, value) of every GPU case, in table order"""
    return [(key, i, v) for key, rows in FORMS.items() for i, r in enumerate(rows) for v in r["values"]]


# ------------------------------------------------------------------------------------------------ exact reduction inputs
# Integer-valued operands: |a_i|, |b_i| <= 2^10 and n <= 2^20, so every product is below 2^20 in magnitude and every partial sum of
# a dot below 2^40: exact in Float64 (and the operands exact in Float32) in ANY summation order. The device scalar must EQUAL
# the int64 result — no tolerance for a grid-changing key to hide a dropped or doubled element in.
DOT_BOUND = 1 << 10
# the six sums of mxlo_diagqn_push include sum s^4 and sum s^2 d: |s_i| <= 2^8, y_i = k_i s_i with 1 <= k_i <= 4, 1 <= d_i <= 16
DQN_S_BOUND, DQN_K, DQN_D = 1 << 8, 4, 16


@functools.lru_cache(maxsize=None)
def int_vectors(n, seed, bound=DOT_BOUND, parts=1):
    """`2 * parts` int64 vectors of length n with entries in [-bound, bound], none of them all zero, read-only"""
    rng = np.random.default_rng(9000 + seed + n)
    out = []
    for _ in range(2 * parts):
        a = rng.integers(-bound, bound + 1, n, dtype=np.int64)
        a[-1] = bound if n % 2 else -bound                        # the tail element carries weight: dropping it shows
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def dot_exact(t, n):
    """(a, b, want): integer operands of mxlo_dot (f64, f32: want an int) or mxlo_dot_c (c128: want = sum conj(a) b, a complex of ints)"""
    if t != "c128":
        a, b = int_vectors(n, 1)
        return a, b, int(np.dot(a, b))
    ar, br, ai, bi = int_vectors(n, 2, parts=2)
    re = int(np.dot(ar, br)) + int(np.dot(ai, bi))
    im = int(np.dot(ar, bi)) - int(np.dot(ai, br))
    return (ar, ai), (br, bi), (re, im)


@functools.lru_cache(maxsize=None)
def diagqn_exact(n, seed=3):
    """(s, y, d, sums): integer operands of mxlo_diagqn_push and its six sums (s^2, s^4, s y, s^2 d, |y|, #(s != 0)) as Python ints"""
    rng = np.random.default_rng(9100 + seed + n)
    s = rng.integers(-DQN_S_BOUND, DQN_S_BOUND + 1, n, dtype=np.int64)
    s[-1] = DQN_S_BOUND
    y = s * rng.integers(1, DQN_K + 1, n, dtype=np.int64)         # s'y > 0
    d = rng.integers(1, DQN_D + 1, n, dtype=np.int64)
    for a in (s, y, d):
        a.setflags(write=False)
    s2 = s * s
    sums = (int(s2.sum()), int((s2 * s2).sum()), int((s * y).sum()), int((s2 * d).sum()), int(np.abs(y).sum()), int((s != 0).sum()))
    return s, y, d, sums


def exact_magnitudes():
    """the largest sum of magnitudes behind any exact comparison of the table: must stay below 2^53 (test_forms_host.py)"""
    worst = 0
    for t, n in DOTS:
        a, b, _ = dot_exact(t, n)
        if t == "c128":
            (ar, ai), (br, bi) = a, b
            worst = max(worst, int((np.abs(ar * br) + np.abs(ai * bi)).sum()), int((np.abs(ar * bi) + np.abs(ai * br)).sum()))
        else:
            worst = max(worst, int(np.abs(a * b).sum()))
    for n in sorted({n for _, _, n in DIAGQN}):
        worst = max(worst, *diagqn_exact(n)[3])
    return worst
