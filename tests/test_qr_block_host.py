"""CPU: the host half of the block form of opQR's apply (`A \\ V` for a rectangular dense A) — the C-ABI entry point
`mxlo_qr_mul_block`, its declaration and prototype, the launch count a matrix apply promises and the grouping constant.
No device call anywhere in this file."""
import inspect
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parents[1]
BLK, VEC = "mxlo_qr_mul_block", "mxlo_qr_mul"


def header_params(name):
    """the parameter names of `name` as include/mxlo.h declares it, in order"""
    src = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "mxlo.h").read_text(), flags=re.S)
    m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/mxlo.h"
    return [re.search(r"(\w+)\s*$", p).group(1) for p in m.group(1).split(",")]


def test_the_entry_point_is_declared_prototyped_and_exported(lo):
    assert BLK in lo._lib.header_symbols()
    assert BLK in lo._lib._PROTOS
    assert hasattr(lo._lib.lib(), BLK)                      # exported by the built library


def test_the_block_prototype_is_the_vector_one_plus_ldr_ldv_and_k(lo):
    """the operand convention of mxlo_gemv_block: ldr follows res; V keeps the place of v and is followed by ldv and k"""
    P = lo._lib._PROTOS
    hv, hb = header_params(VEC), header_params(BLK)
    assert len(hb) == len(hv) + 3 and len(P[BLK]) == len(P[VEC]) + 3
    assert len(P[BLK]) == len(hb)
    want = []
    for p in hv:
        want.append("V" if p == "v" else p)
        if p == "res":
            want.append("ldr")
        if p == "v":
            want += ["ldv", "k"]
    assert hb == want, (hb, want)
    proto = list(P[VEC])                                    # the ctypes of the same positions
    ir, iv = hv.index("res"), hv.index("v")
    proto[iv + 1:iv + 1] = [lo._lib._i64, lo._lib._i64]
    proto[ir + 1:ir + 1] = [lo._lib._i64]
    assert list(P[BLK]) == proto


def test_a_matrix_apply_is_one_chain_per_group_of_eight_columns(lo):
    assert list(inspect.signature(lo.linalg.qr_block_launches).parameters) == ["nf", "k"]
    for nf in (1, 64, 65, 129):
        chain = 2 * -(-nf // 64) + 1
        assert lo.linalg.qr_launches(nf) == chain
        for k in (1, 8, 9, 17):
            got = lo.linalg.qr_block_launches(nf, k)
            assert isinstance(got, int) and got == -(-k // 8) * chain, (nf, k, got)


def test_the_host_group_is_the_kernels(lo):
    src = (ROOT / "linearoperators.jl_amd" / "csrc" / "linalg.hip").read_text()
    kb = re.search(r"constexpr int KB = (\d+);", src)
    assert kb and lo.linalg.GROUP == int(kb.group(1)) == 8
