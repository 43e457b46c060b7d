"""CPU: the host half of the block right-hand-side solves (`F \\ V` for opCholesky, opLDL, opLU and triangular opInverse) —
the four C-ABI entry points, their declarations and prototypes. No device call anywhere in this file."""
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parents[1]
PAIRS = {"mxlo_trisolve_mul_block": "mxlo_trisolve_mul", "mxlo_chol_mul_block": "mxlo_chol_mul",
         "mxlo_ldl_mul_block": "mxlo_ldl_mul", "mxlo_lu_mul_block": "mxlo_lu_mul"}


def header_params(name):
    """the parameter names of `name` as include/mxlo.h declares it, in order"""
    src = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "mxlo.h").read_text(), flags=re.S)
    m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/mxlo.h"
    return [re.search(r"(\w+)\s*$", p).group(1) for p in m.group(1).split(",")]


def test_the_four_entry_points_are_declared_prototyped_and_exported(lo):
    syms = lo._lib.header_symbols()
    L = lo._lib.lib()
    for name in PAIRS:
        assert name in syms, name
        assert name in lo._lib._PROTOS, name
        assert hasattr(L, name), name                       # exported by the built library


def test_each_block_prototype_is_the_vector_one_plus_ldr_ldv_and_k(lo):
    """the operand convention of mxlo_gemv_block: ldr follows res; V keeps the place of v and is followed by ldv and k"""
    P = lo._lib._PROTOS
    for blk, vec in PAIRS.items():
        hv, hb = header_params(vec), header_params(blk)
        assert len(hb) == len(hv) + 3 and len(P[blk]) == len(P[vec]) + 3, blk
        assert len(P[blk]) == len(hb), blk
        want = []
        for p in hv:
            want.append("V" if p == "v" else p)
            if p == "res":
                want.append("ldr")
            if p == "v":
                want += ["ldv", "k"]
        assert hb == want, (blk, hb, want)
        proto = list(P[vec])                                # the ctypes of the same positions
        ir, iv = hv.index("res"), hv.index("v")
        proto[iv + 1:iv + 1] = [lo._lib._i64, lo._lib._i64]
        proto[ir + 1:ir + 1] = [lo._lib._i64]
        assert list(P[blk]) == proto, blk


def test_the_host_mirrors_group_and_block_width_are_the_kernels(lo):
    """linalg.py sizes the work matrix (n x GROUP doubles) and the block inverses (BLOCK x BLOCK) by these two constants; the
    kernel writes n x KB and NB x NB. (The size of an operator's work matrix itself is asserted on the GPU.)"""
    src = (ROOT / "linearoperators.jl_amd" / "csrc" / "linalg.hip").read_text()
    kb = re.search(r"constexpr int KB = (\d+);", src)
    nb = re.search(r"constexpr int NB = (\d+);", src)
    assert kb and nb
    assert lo.linalg.GROUP == int(kb.group(1)) == 8 and lo.linalg.BLOCK == int(nb.group(1)) == 64
