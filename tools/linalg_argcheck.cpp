// Host-side check of the argument checks of the factorisation entry points of linalg.hip: the three factorisations of the
// rectangular family (mxlo_geqrf, mxlo_geqp3, mxlo_cod_factor) and their six applies, mxlo_getrf / mxlo_potrf / mxlo_ldlt, the
// square applies, mxlo_sytrf with its two applies, the snapshot and residual entry points of the refined applies, and one
// common list of cases for both members of each of the eight vector / block pairs of applies. Every call below is refused
// (null operands, bad shapes, a bad rank, overlaps, a scratch one double too short), or is a no-op, before anything touches
// a device, so the program needs no GPU. The pointers are addresses
// inside one host buffer that is never dereferenced by the library. Calls that break two rules at once pin which refusal wins.
// Build the host code with AddressSanitizer and UBSan and run it (from the repository root):
//
//   hipcc -O1 -g -std=c++20 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Iinclude tools/linalg_argcheck.cpp linearoperators.jl_amd/csrc/linalg.hip linearoperators.jl_amd/csrc/api_ctx.hip \
//       -o /tmp/linalg_argcheck && /tmp/linalg_argcheck
//
// info and rank are -1 before every call. A line is `case | status, info, rank | message`; the first two fields are what a
// change of the host code must leave as they are (profiles/linalg_argcheck.txt). Exits 0 when every status is the expected one.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../linearoperators.jl_amd/csrc/common.h"
#include "mxlo.h"

namespace mxlo {                                        // api_ctx.hip (mxlo_last_error) refers to it; the quasi-Newton code is not linked
bool qn_generation(const mxlo_qn *, int64_t *) { return false; }
}

namespace {
constexpr int32_t OK = MXLO_OK, EINVAL_ = MXLO_EINVAL, ESHAPE = MXLO_ESHAPE, ESTATE = MXLO_ESTATE;
constexpr int32_t F64 = MXLO_F64, F32 = MXLO_F32, N = MXLO_OP_N, T = MXLO_OP_T;

// every argument of every entry point under test; a case changes a copy of the valid set
struct Args {
  mxlo_ctx *ctx;
  int32_t dtype = F64, op = N, mtrans = 0, upper = 0, rowmajor = 0, steps = 2;
  int64_t mf = 200, nf = 129, rank = 65, n = 200, k = 8;
  int64_t ldm = 200, ldw = 200, ldr = 129, ldv = 200, lda = 200;      // ldr / ldv: for op N of the rectangular family
  double rtol = 1e-13;
  double *M, *W, *tfac, *dinv, *W2, *tfac2, *dinv2, *scratch, *work, *res, *v;
  double *dinv_u, *d, *dg, *A2;                                       // square family: W, dinv (= dinv_l) and these
  int32_t *jpvt, *info_dev, *info, *rank_out;
  double *e, *panel;                                                  // mxlo_sytrf: the sub-diagonal of D, the n x 65 workspace and
  int32_t *perm;                                                      // its 2 n + ceil(n/64) + 1 words
  double *R, *X;                                                      // the residual entry points: n x k doubles each
  int64_t slen = 0;
  Args tr() const { Args a = *this; a.op = T; a.ldr = mf; a.ldv = nf; return a; }            // the valid transposed apply
  Args sq() const { Args a = *this; a.ldr = a.ldv = n; return a; }                           // the valid square apply
};

int failures = 0, lines = 0;
int32_t info, rank;

template <typename F, typename G>
void expect(const char *what, const Args &base, F &&call, G &&change, int32_t want) {
  Args a = base;
  change(a);
  info = rank = -1;
  const int32_t got = call(a);
  std::printf("%-62s | status %d info %d rank %d | %s%s\n", what, got, info, rank, got ? mxlo_last_error() : "ok",
              got == want ? "" : "   <-- UNEXPECTED");
  ++lines;
  if (got != want) ++failures;
}

int32_t geqrf(const Args &a) { return mxlo_geqrf(a.ctx, a.dtype, a.M, a.ldm, a.mtrans, a.W, a.ldw, a.mf, a.nf, a.tfac, a.dinv, a.scratch, a.slen, a.info_dev, a.info); }
int32_t qr_mul(const Args &a) { return mxlo_qr_mul(a.ctx, a.dtype, a.res, a.W, a.ldw, a.mf, a.nf, a.tfac, a.dinv, a.work, a.v, a.op, 1.0, 0.0); }
int32_t qr_mul_block(const Args &a) { return mxlo_qr_mul_block(a.ctx, a.dtype, a.res, a.ldr, a.W, a.ldw, a.mf, a.nf, a.tfac, a.dinv, a.work, a.v, a.ldv, a.k, a.op, 1.0, 0.0); }
int32_t geqp3(const Args &a) { return mxlo_geqp3(a.ctx, a.dtype, a.M, a.ldm, a.mtrans, a.W, a.ldw, a.mf, a.nf, a.tfac, a.dinv, a.jpvt, a.rtol, a.scratch, a.slen, a.info_dev, a.info, a.rank_out); }
int32_t qrp_mul(const Args &a) { return mxlo_qrp_mul(a.ctx, a.dtype, a.res, a.W, a.ldw, a.mf, a.nf, a.tfac, a.dinv, a.jpvt, a.rank, a.work, a.v, a.op, 1.0, 0.0); }
int32_t qrp_mul_block(const Args &a) { return mxlo_qrp_mul_block(a.ctx, a.dtype, a.res, a.ldr, a.W, a.ldw, a.mf, a.nf, a.tfac, a.dinv, a.jpvt, a.rank, a.work, a.v, a.ldv, a.k, a.op, 1.0, 0.0); }
int32_t cod_factor(const Args &a) { return mxlo_cod_factor(a.ctx, a.dtype, a.W, a.ldw, a.nf, a.rank, a.W2, a.tfac2, a.dinv2, a.scratch, a.slen, a.info_dev, a.info); }
int32_t pinv_mul(const Args &a) { return mxlo_pinv_mul(a.ctx, a.dtype, a.res, a.W, a.ldw, a.mf, a.nf, a.tfac, a.jpvt, a.rank, a.W2, a.tfac2, a.dinv2, a.work, a.v, a.op, 1.0, 0.0); }
int32_t pinv_mul_block(const Args &a) { return mxlo_pinv_mul_block(a.ctx, a.dtype, a.res, a.ldr, a.W, a.ldw, a.mf, a.nf, a.tfac, a.jpvt, a.rank, a.W2, a.tfac2, a.dinv2, a.work, a.v, a.ldv, a.k, a.op, 1.0, 0.0); }
int32_t getrf(const Args &a) { return mxlo_getrf(a.ctx, a.dtype, a.M, a.ldm, a.W, a.ldw, a.n, a.dinv, a.dinv_u, a.jpvt, a.info_dev, a.info); }
int32_t potrf(const Args &a) { return mxlo_potrf(a.ctx, a.dtype, a.M, a.ldm, a.rowmajor, a.W, a.ldw, a.n, a.dinv, a.info_dev, a.info); }
int32_t ldlt(const Args &a) { return mxlo_ldlt(a.ctx, a.dtype, a.M, a.ldm, a.rowmajor, a.W, a.ldw, a.n, a.dinv, a.d, a.info_dev, a.info); }
int32_t trisolve_mul_block(const Args &a) { return mxlo_trisolve_mul_block(a.ctx, a.dtype, a.res, a.ldr, a.W, a.ldw, a.n, a.upper, a.op, a.dinv, a.work, a.v, a.ldv, a.k, 1.0, 0.0); }
int32_t chol_mul(const Args &a) { return mxlo_chol_mul(a.ctx, a.dtype, a.res, a.W, a.ldw, a.n, a.dinv, a.work, a.v, 1.0, 0.0); }
int32_t sym_snapshot(const Args &a) { return mxlo_sym_snapshot(a.ctx, a.dtype, a.M, a.ldm, a.rowmajor, a.W, a.ldw, a.n, a.dg); }
int32_t lu_snapshot(const Args &a) { return mxlo_lu_snapshot(a.ctx, a.dtype, a.M, a.ldm, a.jpvt, a.A2, a.lda, a.n); }
int32_t sym_residual(const Args &a) { return mxlo_sym_residual(a.ctx, a.dtype, a.R, a.W, a.ldw, a.dg, a.n, a.v, a.ldv, a.X, a.k); }
int32_t gen_residual(const Args &a) { return mxlo_gen_residual(a.ctx, a.dtype, a.R, a.A2, a.lda, a.n, a.v, a.ldv, a.X, a.k, a.op); }
int32_t trisolve_mul(const Args &a) { return mxlo_trisolve_mul(a.ctx, a.dtype, a.res, a.W, a.ldw, a.n, a.upper, a.op, a.dinv, a.work, a.v, 1.0, 0.0); }
int32_t chol_mul_block(const Args &a) { return mxlo_chol_mul_block(a.ctx, a.dtype, a.res, a.ldr, a.W, a.ldw, a.n, a.dinv, a.work, a.v, a.ldv, a.k, 1.0, 0.0); }
int32_t ldl_mul(const Args &a) { return mxlo_ldl_mul(a.ctx, a.dtype, a.res, a.W, a.ldw, a.n, a.dinv, a.d, a.work, a.v, 1.0, 0.0); }
int32_t ldl_mul_block(const Args &a) { return mxlo_ldl_mul_block(a.ctx, a.dtype, a.res, a.ldr, a.W, a.ldw, a.n, a.dinv, a.d, a.work, a.v, a.ldv, a.k, 1.0, 0.0); }
int32_t lu_mul(const Args &a) { return mxlo_lu_mul(a.ctx, a.dtype, a.res, a.W, a.ldw, a.n, a.dinv, a.dinv_u, a.jpvt, a.work, a.v, a.op, 1.0, 0.0); }
int32_t lu_mul_block(const Args &a) { return mxlo_lu_mul_block(a.ctx, a.dtype, a.res, a.ldr, a.W, a.ldw, a.n, a.dinv, a.dinv_u, a.jpvt, a.work, a.v, a.ldv, a.k, a.op, 1.0, 0.0); }
int32_t ldl_mul_refine(const Args &a) { return mxlo_ldl_mul_refine(a.ctx, a.dtype, a.res, a.ldr, a.W, a.ldw, a.n, a.dinv, a.d, a.dg, a.work, a.v, a.ldv, a.k, a.steps, 1.0, 0.0); }
int32_t lu_mul_refine(const Args &a) { return mxlo_lu_mul_refine(a.ctx, a.dtype, a.res, a.ldr, a.W, a.ldw, a.n, a.dinv, a.dinv_u, a.jpvt, a.A2, a.lda, a.work, a.v, a.ldv, a.k, a.steps, a.op, 1.0, 0.0); }
int32_t sytrf(const Args &a) { return mxlo_sytrf(a.ctx, a.dtype, a.M, a.ldm, a.rowmajor, a.W, a.ldw, a.n, a.dinv, a.d, a.e, a.perm, a.panel, a.info_dev, a.info); }
int32_t ldlp_mul(const Args &a) { return mxlo_ldlp_mul(a.ctx, a.dtype, a.res, a.W, a.ldw, a.n, a.dinv, a.d, a.e, a.perm, a.work, a.v, 1.0, 0.0); }
int32_t ldlp_mul_block(const Args &a) { return mxlo_ldlp_mul_block(a.ctx, a.dtype, a.res, a.ldr, a.W, a.ldw, a.n, a.dinv, a.d, a.e, a.perm, a.work, a.v, a.ldv, a.k, 1.0, 0.0); }

// What both members of a vector / block pair of applies are asked, so that the two forms of an operator cannot drift apart:
// null res, null V, a leading dimension one too small, res overlapping the factor, res overlapping V without being V, the
// no-ops, and calls that break two rules. sq: the square family (n, ldw), else the rectangular one (mf, nf, ldw; op N, whose
// res has nf rows). A vector entry point has no ldr / ldv and no k: its no-op is n == 0, which the rectangular family refuses.
template <typename F>
void pair_cases(const char *name, const Args &base, F &&call, bool block, bool sq) {
  char what[96];
  auto run = [&](const char *c, int32_t want, auto &&change) {
    std::snprintf(what, sizeof what, "%s, pair: %s", name, c);
    expect(what, base, call, change, want);
  };
  const int64_t rows = sq ? base.n : base.mf;
  run("null res", EINVAL_, [](Args &a) { a.res = nullptr; });
  run("null V", EINVAL_, [](Args &a) { a.v = nullptr; });
  run("the factor's ld one too small", ESHAPE, [&](Args &a) { a.ldw = rows - 1; });
  run("res overlaps the factor", EINVAL_, [](Args &a) { a.res = a.W + 3; });
  run("res ends at the factor's first element", EINVAL_, [&](Args &a) { a.res = a.W - (block ? (a.k - 1) * a.ldr : 0) - (sq ? a.n : a.nf) + 1; });
  run("res overlaps V without being V", EINVAL_, [](Args &a) { a.res = a.v + 1; });
  run("float: res overlaps V without being V", EINVAL_, [](Args &a) { a.dtype = F32; a.res = (double *)((float *)a.v + 1); });
  run("ld too small + null res", ESHAPE, [&](Args &a) { a.ldw = rows - 1; a.res = nullptr; });
  run("null V + res overlaps the factor", EINVAL_, [](Args &a) { a.v = nullptr; a.res = a.W + 3; });
  run("res overlaps V + res overlaps the factor", EINVAL_, [](Args &a) { a.v = a.W + 1; a.res = a.W + 3; });
  if (sq) {
    run("n == 0 launches nothing", OK, [](Args &a) { a.n = 0; a.res = nullptr; a.v = nullptr; a.W = nullptr; });
    run("n == 0 + ld 0", ESHAPE, [](Args &a) { a.n = 0; a.ldw = 0; });
  } else {
    run("nf == 0 is no no-op", ESHAPE, [](Args &a) { a.nf = 0; a.res = nullptr; a.v = nullptr; });
  }
  if (block) {
    run("ldr one too small", ESHAPE, [&](Args &a) { a.ldr = (sq ? a.n : a.nf) - 1; });
    run("ldv one too small", ESHAPE, [&](Args &a) { a.ldv = rows - 1; });
    run("k == 0 launches nothing", OK, [](Args &a) { a.k = 0; a.res = nullptr; a.v = nullptr; });
    run("k == 0 + ldr one too small", ESHAPE, [&](Args &a) { a.k = 0; a.ldr = (sq ? a.n : a.nf) - 1; });
    run("ldv one too small + null V", ESHAPE, [&](Args &a) { a.ldv = rows - 1; a.v = nullptr; });
    run("res is V in another leading dimension", EINVAL_, [](Args &a) { a.res = a.v; a.ldv = a.ldv + 1; a.k = 7; });
  }
}
}  // namespace

#define CASE(what, base, call, want, ...) expect(what, base, call, [&](Args &a) { __VA_ARGS__; }, want)

int main() {
  mxlo_ctx ctx;                                         // never used for a launch: every call returns before the device guard
  const int64_t mf = 200, nf = 129, r = 65, n = 200, QS = 512 * 64;
  const int64_t geqrf_len = 2 * (QS + 64) + (512 + 2 * 3) * 4096;            // nf = 129: three block columns
  const int64_t geqp3_len = 2 * 64 * nf + 64 + 2 * nf + 2 * mf + 2 + 64 * 4096;
  const int64_t cod_len = 2 * (QS + 64) + (512 + 2 * 2) * 4096;              // rank 65: two block columns
  const int64_t work_len = 8 * (mf + nf + 2 * QS);
  std::vector<double> pool(3 * n * n + mf * nf + nf * r + 8 * 4 * 4096 + nf + geqrf_len + work_len + 16 * mf + 3 * n + 4096 + 66 * n + 3 * n);
  double *p = pool.data();
  Args b;
  b.ctx = &ctx;
  b.M = p; p += n * n;                                  // the square family's n x n; the rectangular one's mf x nf
  b.W = p; p += n * n;
  b.A2 = p; p += n * n;
  b.tfac = p; p += 4 * 4096;
  b.dinv = p; p += 4 * 4096;
  b.dinv_u = p; p += 4 * 4096;
  b.jpvt = (int32_t *)p; p += n;                        // also getrf's permutation, which it sizes as 8 n bytes
  b.W2 = p; p += nf * r;
  b.tfac2 = p; p += 4 * 4096;
  b.dinv2 = p; p += 4 * 4096;
  b.d = p; p += n;
  b.dg = p; p += n;
  b.scratch = p; p += geqrf_len;
  b.info_dev = (int32_t *)p; p += 1;
  b.work = p; p += work_len;
  b.res = p; p += 8 * mf;
  b.v = p; p += 8 * mf;
  p += 3 * n + 4096 - 1;                                // the slack the pool always had; what mxlo_sytrf adds lies behind it
  b.e = p; p += n;
  b.panel = p; p += 65 * n;
  b.perm = (int32_t *)p; p += n + 3;                    // 2 n + 4 + 1 words
  b.R = b.work;                                         // the residual entry points borrow the work space: 8 n doubles each
  b.X = b.work + 8 * n;
  b.info = &info;
  b.rank_out = &rank;
  double *const M = b.M, *const W = b.W, *const W2 = b.W2, *const tfac2 = b.tfac2, *const dinv2 = b.dinv2, *const scratch = b.scratch;
  double *const work = b.work, *const res = b.res, *const v = b.v, *const dinv = b.dinv, *const tfac = b.tfac;
  int32_t *const jpvt = b.jpvt;
  const Args bt = b.tr(), s = b.sq();                   // the transposed rectangular apply; the square apply
  Args g = b;

  // ---- mxlo_geqrf
  g = b; g.slen = geqrf_len;
  CASE("geqrf: null ctx", g, geqrf, EINVAL_, a.ctx = nullptr);
  CASE("geqrf: complex dtype", g, geqrf, EINVAL_, a.dtype = MXLO_C64);
  CASE("geqrf: nf > mf", g, geqrf, ESHAPE, a.mf = nf; a.nf = mf);
  CASE("geqrf: nf == 0", g, geqrf, ESHAPE, a.nf = 0);
  CASE("geqrf: ldw < mf", g, geqrf, ESHAPE, a.ldw = mf - 1);
  CASE("geqrf: mf too large", g, geqrf, ESHAPE, a.mf = a.ldw = a.ldm = 1LL << 31);
  CASE("geqrf: null M", g, geqrf, EINVAL_, a.M = nullptr);
  CASE("geqrf: null dinv", g, geqrf, EINVAL_, a.dinv = nullptr);
  CASE("geqrf: null info", g, geqrf, EINVAL_, a.info = nullptr);
  CASE("geqrf: ldm < mf leaves info 0", g, geqrf, ESHAPE, a.ldm = mf - 1);
  CASE("geqrf: ldm < nf, transposed", g, geqrf, ESHAPE, a.mtrans = 1; a.ldm = nf - 1);
  CASE("geqrf: scratch one double too short", g, geqrf, ESHAPE, a.slen = geqrf_len - 1);
  CASE("geqrf: W is M", g, geqrf, EINVAL_, a.W = M);
  CASE("geqrf: tfac inside W", g, geqrf, EINVAL_, a.tfac = W + 7);
  CASE("geqrf: dinv is tfac", g, geqrf, EINVAL_, a.dinv = tfac);
  CASE("geqrf: info word inside the scratch", g, geqrf, EINVAL_, a.info_dev = (int32_t *)scratch + 5);
  CASE("geqrf: M transposed ends inside W", g, geqrf, EINVAL_, a.mtrans = 1; a.ldm = nf; a.M = W - nf * mf + 1);
  ctx.capturing = true;
  CASE("geqrf: during a capture", g, geqrf, ESTATE, (void)a);
  CASE("geqrf: during a capture, float", g, geqrf, ESTATE, a.dtype = F32);
  ctx.capturing = false;
  CASE("geqrf: bad dtype + bad shape", g, geqrf, EINVAL_, a.dtype = MXLO_C64; a.nf = 0);
  CASE("geqrf: bad shape + null operand", g, geqrf, ESHAPE, a.ldw = 1; a.W = nullptr);
  CASE("geqrf: too large + null info", g, geqrf, ESHAPE, a.mf = a.ldw = a.ldm = 1LL << 31; a.info = nullptr);
  CASE("geqrf: null operand + bad ldm leaves info untouched", g, geqrf, EINVAL_, a.tfac = nullptr; a.ldm = 1);
  CASE("geqrf: bad ldm + short scratch", g, geqrf, ESHAPE, a.ldm = 1; a.slen = 0);
  CASE("geqrf: short scratch + overlap", g, geqrf, ESHAPE, a.slen = geqrf_len - 1; a.W = M);
  ctx.capturing = true;
  CASE("geqrf: overlap + capture", g, geqrf, EINVAL_, a.W = M);
  ctx.capturing = false;

  // ---- mxlo_qr_mul
  CASE("qr_mul: null ctx", b, qr_mul, EINVAL_, a.ctx = nullptr);
  CASE("qr_mul: complex dtype", b, qr_mul, EINVAL_, a.dtype = MXLO_C64);
  CASE("qr_mul: bad op_mode", b, qr_mul, EINVAL_, a.op = 77);
  CASE("qr_mul: nf > mf", b, qr_mul, ESHAPE, a.mf = nf; a.nf = mf);
  CASE("qr_mul: nf == 0", b, qr_mul, ESHAPE, a.nf = 0);
  CASE("qr_mul: ldw < mf", b, qr_mul, ESHAPE, a.ldw = mf - 1);
  CASE("qr_mul: mf too large", b, qr_mul, ESHAPE, a.mf = a.ldw = 1LL << 31);
  CASE("qr_mul: null res", b, qr_mul, EINVAL_, a.res = nullptr);
  CASE("qr_mul: null v", b, qr_mul, EINVAL_, a.v = nullptr);
  CASE("qr_mul: null tfac", b, qr_mul, EINVAL_, a.tfac = nullptr);
  CASE("qr_mul: null work", b, qr_mul, EINVAL_, a.work = nullptr);
  CASE("qr_mul: res is v, rectangular", b, qr_mul, EINVAL_, a.res = v);
  CASE("qr_mul: res overlaps v, transposed", bt, qr_mul, EINVAL_, a.res = v + 1);
  CASE("qr_mul: res inside W", b, qr_mul, EINVAL_, a.res = W + 11);
  CASE("qr_mul: v ends inside tfac", b, qr_mul, EINVAL_, a.v = tfac - mf + 1);
  CASE("qr_mul: res inside dinv, float", b, qr_mul, EINVAL_, a.dtype = F32; a.res = dinv + 3 * 4096 - 1);
  CASE("qr_mul: res inside the work vector", b, qr_mul, EINVAL_, a.res = work + mf + 2 * QS - 1);
  CASE("qr_mul: bad dtype + bad shape", b, qr_mul, EINVAL_, a.dtype = 9; a.nf = 0);
  CASE("qr_mul: bad op_mode + bad shape", b, qr_mul, EINVAL_, a.op = 77; a.ldw = 1);
  CASE("qr_mul: bad shape + null operand", b, qr_mul, ESHAPE, a.nf = 0; a.res = nullptr);
  CASE("qr_mul: negative mf + null operand", b, qr_mul, ESHAPE, a.mf = -5; a.work = nullptr);
  CASE("qr_mul: null operand + overlap", b, qr_mul, EINVAL_, a.tfac = nullptr; a.res = W);

  // ---- mxlo_qr_mul_block
  CASE("qr_mul_block: null ctx", b, qr_mul_block, EINVAL_, a.ctx = nullptr);
  CASE("qr_mul_block: complex dtype", b, qr_mul_block, EINVAL_, a.dtype = MXLO_C32);
  CASE("qr_mul_block: bad op_mode", b, qr_mul_block, EINVAL_, a.op = -1);
  CASE("qr_mul_block: nf > mf", b, qr_mul_block, ESHAPE, a.mf = nf; a.nf = mf);
  CASE("qr_mul_block: k == 0 launches nothing", b, qr_mul_block, OK, a.k = 0; a.res = nullptr; a.v = nullptr);
  CASE("qr_mul_block: k < 0", b, qr_mul_block, ESHAPE, a.k = -1);
  CASE("qr_mul_block: ldr < nf", b, qr_mul_block, ESHAPE, a.ldr = nf - 1);
  CASE("qr_mul_block: ldv < mf", b, qr_mul_block, ESHAPE, a.ldv = mf - 1);
  CASE("qr_mul_block: ldv < nf, transposed", bt, qr_mul_block, ESHAPE, a.ldv = nf - 1);
  CASE("qr_mul_block: ldr < mf, transposed", bt, qr_mul_block, ESHAPE, a.ldr = mf - 1);
  CASE("qr_mul_block: null dinv", b, qr_mul_block, EINVAL_, a.dinv = nullptr);
  CASE("qr_mul_block: null V", b, qr_mul_block, EINVAL_, a.v = nullptr);
  CASE("qr_mul_block: res is V, rectangular", b, qr_mul_block, EINVAL_, a.res = v; a.ldr = mf);
  CASE("qr_mul_block: last column of res inside tfac", b, qr_mul_block, EINVAL_, a.res = tfac - 7 * nf);
  CASE("qr_mul_block: V inside W, transposed", bt, qr_mul_block, EINVAL_, a.v = W);
  CASE("qr_mul_block: res inside the work space", b, qr_mul_block, EINVAL_, a.res = work + 8 * (mf + nf) + 5);
  CASE("qr_mul_block: res ends at the work space's last double", b, qr_mul_block, EINVAL_, a.res = work + work_len - 1);
  CASE("qr_mul_block: k == 0 + null operand", b, qr_mul_block, OK, a.k = 0; a.W = nullptr; a.tfac = nullptr);
  CASE("qr_mul_block: k == 0 + bad ldr", b, qr_mul_block, ESHAPE, a.k = 0; a.ldr = 1);
  CASE("qr_mul_block: k == 0 + bad shape", b, qr_mul_block, ESHAPE, a.k = 0; a.nf = 0);
  CASE("qr_mul_block: k == 0 + bad op_mode", b, qr_mul_block, EINVAL_, a.k = 0; a.op = 77);
  CASE("qr_mul_block: bad dtype + bad shape", b, qr_mul_block, EINVAL_, a.dtype = 9; a.mf = 0);
  CASE("qr_mul_block: bad shape + null operand", b, qr_mul_block, ESHAPE, a.ldv = 0; a.v = nullptr);
  CASE("qr_mul_block: null operand + overlap", b, qr_mul_block, EINVAL_, a.work = nullptr; a.res = W);

  // ---- mxlo_geqp3
  g = b; g.slen = geqp3_len;
  CASE("geqp3: null ctx", g, geqp3, EINVAL_, a.ctx = nullptr);
  CASE("geqp3: complex dtype", g, geqp3, EINVAL_, a.dtype = MXLO_C64);
  CASE("geqp3: nf > mf", g, geqp3, ESHAPE, a.mf = nf; a.nf = mf);
  CASE("geqp3: nf == 0", g, geqp3, ESHAPE, a.nf = 0);
  CASE("geqp3: ldw < mf", g, geqp3, ESHAPE, a.ldw = mf - 1);
  CASE("geqp3: mf too large", g, geqp3, ESHAPE, a.mf = a.ldw = a.ldm = 1LL << 31);
  CASE("geqp3: rtol == 1", g, geqp3, EINVAL_, a.rtol = 1.0);
  CASE("geqp3: rtol < 0", g, geqp3, EINVAL_, a.rtol = -1e-3);
  CASE("geqp3: rtol NaN", g, geqp3, EINVAL_, a.rtol = __builtin_nan(""));
  CASE("geqp3: null M", g, geqp3, EINVAL_, a.M = nullptr);
  CASE("geqp3: null jpvt", g, geqp3, EINVAL_, a.jpvt = nullptr);
  CASE("geqp3: null rank", g, geqp3, EINVAL_, a.rank_out = nullptr);
  CASE("geqp3: null info", g, geqp3, EINVAL_, a.info = nullptr);
  CASE("geqp3: ldm < mf", g, geqp3, ESHAPE, a.ldm = mf - 1);
  CASE("geqp3: ldm < nf, transposed", g, geqp3, ESHAPE, a.mtrans = 1; a.ldm = nf - 1);
  CASE("geqp3: scratch one double too short", g, geqp3, ESHAPE, a.slen = geqp3_len - 1);
  CASE("geqp3: W is M", g, geqp3, EINVAL_, a.W = M);
  CASE("geqp3: jpvt inside W", g, geqp3, EINVAL_, a.jpvt = (int32_t *)(W + 7));
  CASE("geqp3: jpvt inside the scratch", g, geqp3, EINVAL_, a.jpvt = (int32_t *)scratch + 5);
  CASE("geqp3: second info word inside jpvt", g, geqp3, EINVAL_, a.info_dev = jpvt - 1);
  ctx.capturing = true;
  CASE("geqp3: during a capture", g, geqp3, ESTATE, (void)a);
  CASE("geqp3: overlap + capture", g, geqp3, EINVAL_, a.dinv = tfac);
  ctx.capturing = false;
  CASE("geqp3: bad dtype + bad shape", g, geqp3, EINVAL_, a.dtype = MXLO_C64; a.nf = 0);
  CASE("geqp3: bad shape + bad rtol", g, geqp3, ESHAPE, a.nf = 0; a.rtol = 2.0);
  CASE("geqp3: bad rtol + null operand", g, geqp3, EINVAL_, a.rtol = 2.0; a.M = nullptr);
  CASE("geqp3: null rank + bad ldm leaves info untouched", g, geqp3, EINVAL_, a.rank_out = nullptr; a.ldm = 1);
  CASE("geqp3: bad ldm + overlap leaves info, rank 0", g, geqp3, ESHAPE, a.ldm = 1; a.W = M);
  CASE("geqp3: short scratch + overlap", g, geqp3, ESHAPE, a.slen = 0; a.W = M);

  // ---- mxlo_qrp_mul
  CASE("qrp_mul: null ctx", b, qrp_mul, EINVAL_, a.ctx = nullptr);
  CASE("qrp_mul: bad op_mode", b, qrp_mul, EINVAL_, a.op = 77);
  CASE("qrp_mul: nf > mf", b, qrp_mul, ESHAPE, a.mf = nf; a.nf = mf);
  CASE("qrp_mul: rank 0", b, qrp_mul, ESHAPE, a.rank = 0);
  CASE("qrp_mul: rank > nf", b, qrp_mul, ESHAPE, a.rank = nf + 1);
  CASE("qrp_mul: null jpvt", b, qrp_mul, EINVAL_, a.jpvt = nullptr);
  CASE("qrp_mul: null res", b, qrp_mul, EINVAL_, a.res = nullptr);
  CASE("qrp_mul: res is v, rectangular", b, qrp_mul, EINVAL_, a.res = v);
  CASE("qrp_mul: res overlaps v", bt, qrp_mul, EINVAL_, a.res = v + 1);
  CASE("qrp_mul: res inside jpvt", b, qrp_mul, EINVAL_, a.res = (double *)jpvt);
  CASE("qrp_mul: v inside jpvt", b, qrp_mul, EINVAL_, a.v = (double *)jpvt - mf + 1);
  CASE("qrp_mul: res inside the work vector", b, qrp_mul, EINVAL_, a.res = work + 3);
  CASE("qrp_mul: res in the third block of tfac (sized by nf, not the rank)", b, qrp_mul, EINVAL_, a.res = tfac + 3 * 4096 - nf);
  CASE("qrp_mul: bad dtype + bad rank", b, qrp_mul, EINVAL_, a.dtype = 9; a.rank = 0);
  CASE("qrp_mul: bad shape + bad rank", b, qrp_mul, ESHAPE, a.nf = 0; a.rank = -1);
  CASE("qrp_mul: bad rank + null operand", b, qrp_mul, ESHAPE, a.rank = nf + 1; a.v = nullptr);
  CASE("qrp_mul: null operand + overlap", b, qrp_mul, EINVAL_, a.jpvt = nullptr; a.res = W);

  // ---- mxlo_qrp_mul_block
  CASE("qrp_mul_block: null ctx", b, qrp_mul_block, EINVAL_, a.ctx = nullptr);
  CASE("qrp_mul_block: k == 0 launches nothing", b, qrp_mul_block, OK, a.k = 0; a.res = nullptr; a.v = nullptr);
  CASE("qrp_mul_block: k < 0", b, qrp_mul_block, ESHAPE, a.k = -1);
  CASE("qrp_mul_block: ldr < nf", b, qrp_mul_block, ESHAPE, a.ldr = nf - 1);
  CASE("qrp_mul_block: ldv < nf, transposed", bt, qrp_mul_block, ESHAPE, a.ldv = nf - 1);
  CASE("qrp_mul_block: rank > nf", b, qrp_mul_block, ESHAPE, a.rank = nf + 1);
  CASE("qrp_mul_block: null jpvt", b, qrp_mul_block, EINVAL_, a.jpvt = nullptr);
  CASE("qrp_mul_block: null V", b, qrp_mul_block, EINVAL_, a.v = nullptr);
  CASE("qrp_mul_block: res is V, rectangular", b, qrp_mul_block, EINVAL_, a.res = v; a.ldr = mf);
  CASE("qrp_mul_block: last column of res inside jpvt", b, qrp_mul_block, EINVAL_, a.res = (double *)jpvt - 7 * nf);
  CASE("qrp_mul_block: V inside jpvt", bt, qrp_mul_block, EINVAL_, a.v = (double *)jpvt);
  CASE("qrp_mul_block: res inside the work space", b, qrp_mul_block, EINVAL_, a.res = work + 8 * (mf + nf) + 5);
  CASE("qrp_mul_block: k == 0 + null operand", b, qrp_mul_block, OK, a.k = 0; a.jpvt = nullptr);
  CASE("qrp_mul_block: k == 0 + bad rank", b, qrp_mul_block, ESHAPE, a.k = 0; a.rank = 0);
  CASE("qrp_mul_block: bad rank + bad ldr", b, qrp_mul_block, ESHAPE, a.rank = 0; a.ldr = 1);
  CASE("qrp_mul_block: bad ldr + null operand", b, qrp_mul_block, ESHAPE, a.ldr = 1; a.res = nullptr);
  CASE("qrp_mul_block: bad op_mode + bad rank", b, qrp_mul_block, EINVAL_, a.op = 77; a.rank = 0);
  CASE("qrp_mul_block: null operand + overlap", b, qrp_mul_block, EINVAL_, a.dinv = nullptr; a.v = W);

  // ---- mxlo_cod_factor
  g = b; g.slen = cod_len;
  CASE("cod_factor: null ctx", g, cod_factor, EINVAL_, a.ctx = nullptr);
  CASE("cod_factor: complex dtype", g, cod_factor, EINVAL_, a.dtype = MXLO_C64);
  CASE("cod_factor: nf == 0", g, cod_factor, ESHAPE, a.nf = 0);
  CASE("cod_factor: ldw < nf", g, cod_factor, ESHAPE, a.ldw = nf - 1);
  CASE("cod_factor: nf too large", g, cod_factor, ESHAPE, a.nf = a.ldw = 1LL << 31);
  CASE("cod_factor: rank 0", g, cod_factor, ESHAPE, a.rank = 0);
  CASE("cod_factor: rank > nf", g, cod_factor, ESHAPE, a.rank = nf + 1);
  CASE("cod_factor: null W", g, cod_factor, EINVAL_, a.W = nullptr);
  CASE("cod_factor: null W2", g, cod_factor, EINVAL_, a.W2 = nullptr);
  CASE("cod_factor: null dinv2", g, cod_factor, EINVAL_, a.dinv2 = nullptr);
  CASE("cod_factor: null info", g, cod_factor, EINVAL_, a.info = nullptr);
  CASE("cod_factor: scratch one double too short", g, cod_factor, ESHAPE, a.slen = cod_len - 1);
  CASE("cod_factor: W2 is W", g, cod_factor, EINVAL_, a.W2 = W);
  CASE("cod_factor: W2 starts in the last column of W", g, cod_factor, EINVAL_, a.W2 = W + (nf - 1) * mf + r - 1);
  CASE("cod_factor: tfac2 inside W2", g, cod_factor, EINVAL_, a.tfac2 = W2 + 7);
  CASE("cod_factor: dinv2 is tfac2", g, cod_factor, EINVAL_, a.dinv2 = tfac2);
  CASE("cod_factor: info word inside the scratch", g, cod_factor, EINVAL_, a.info_dev = (int32_t *)scratch + 5);
  ctx.capturing = true;
  CASE("cod_factor: during a capture", g, cod_factor, ESTATE, (void)a);
  ctx.capturing = false;
  CASE("cod_factor: bad dtype + bad shape", g, cod_factor, EINVAL_, a.dtype = 9; a.nf = 0);
  CASE("cod_factor: bad shape + bad rank", g, cod_factor, ESHAPE, a.ldw = 1; a.rank = 0);
  CASE("cod_factor: bad rank + null operand", g, cod_factor, ESHAPE, a.rank = nf + 1; a.W2 = nullptr);
  CASE("cod_factor: null operand + short scratch leaves info untouched", g, cod_factor, EINVAL_, a.tfac2 = nullptr; a.slen = 0);
  CASE("cod_factor: short scratch + overlap leaves info 0", g, cod_factor, ESHAPE, a.slen = cod_len - 1; a.W2 = W);

  // ---- mxlo_pinv_mul
  CASE("pinv_mul: null ctx", b, pinv_mul, EINVAL_, a.ctx = nullptr);
  CASE("pinv_mul: complex dtype", b, pinv_mul, EINVAL_, a.dtype = MXLO_C64);
  CASE("pinv_mul: bad op_mode", b, pinv_mul, EINVAL_, a.op = 77);
  CASE("pinv_mul: nf > mf", b, pinv_mul, ESHAPE, a.mf = nf; a.nf = mf);
  CASE("pinv_mul: ldw < mf", b, pinv_mul, ESHAPE, a.ldw = mf - 1);
  CASE("pinv_mul: rank 0", b, pinv_mul, ESHAPE, a.rank = 0);
  CASE("pinv_mul: rank == nf", b, pinv_mul, ESHAPE, a.rank = nf);
  CASE("pinv_mul: null jpvt", b, pinv_mul, EINVAL_, a.jpvt = nullptr);
  CASE("pinv_mul: null W2", b, pinv_mul, EINVAL_, a.W2 = nullptr);
  CASE("pinv_mul: null dinv2", b, pinv_mul, EINVAL_, a.dinv2 = nullptr);
  CASE("pinv_mul: null res", b, pinv_mul, EINVAL_, a.res = nullptr);
  CASE("pinv_mul: res is v, rectangular", b, pinv_mul, EINVAL_, a.res = v);
  CASE("pinv_mul: res overlaps v", bt, pinv_mul, EINVAL_, a.res = v + 1);
  CASE("pinv_mul: res inside jpvt", b, pinv_mul, EINVAL_, a.res = (double *)jpvt);
  CASE("pinv_mul: res inside W2", b, pinv_mul, EINVAL_, a.res = W2 + nf * r - 1);
  CASE("pinv_mul: v inside dinv2", b, pinv_mul, EINVAL_, a.v = dinv2 + 9);
  CASE("pinv_mul: v ends inside tfac2", b, pinv_mul, EINVAL_, a.v = tfac2 - mf + 1);
  CASE("pinv_mul: res inside the work vector", b, pinv_mul, EINVAL_, a.res = work + mf + 2 * QS - 1);
  CASE("pinv_mul: negative mf + null operand", b, pinv_mul, ESHAPE, a.mf = -5; a.work = nullptr);
  CASE("pinv_mul: bad dtype + bad rank", b, pinv_mul, EINVAL_, a.dtype = 9; a.rank = nf);
  CASE("pinv_mul: bad shape + bad rank", b, pinv_mul, ESHAPE, a.ldw = 1; a.rank = 0);
  CASE("pinv_mul: bad rank + null operand", b, pinv_mul, ESHAPE, a.rank = nf; a.W2 = nullptr);
  CASE("pinv_mul: null operand + overlap", b, pinv_mul, EINVAL_, a.tfac2 = nullptr; a.res = W);

  // ---- mxlo_pinv_mul_block
  CASE("pinv_mul_block: null ctx", b, pinv_mul_block, EINVAL_, a.ctx = nullptr);
  CASE("pinv_mul_block: k == 0 launches nothing", b, pinv_mul_block, OK, a.k = 0; a.res = nullptr; a.v = nullptr);
  CASE("pinv_mul_block: k < 0", b, pinv_mul_block, ESHAPE, a.k = -1);
  CASE("pinv_mul_block: ldr < nf", b, pinv_mul_block, ESHAPE, a.ldr = nf - 1);
  CASE("pinv_mul_block: ldv < nf, transposed", bt, pinv_mul_block, ESHAPE, a.ldv = nf - 1);
  CASE("pinv_mul_block: rank == nf", b, pinv_mul_block, ESHAPE, a.rank = nf);
  CASE("pinv_mul_block: rank < 1", b, pinv_mul_block, ESHAPE, a.rank = -3);
  CASE("pinv_mul_block: null tfac2", b, pinv_mul_block, EINVAL_, a.tfac2 = nullptr);
  CASE("pinv_mul_block: null V", b, pinv_mul_block, EINVAL_, a.v = nullptr);
  CASE("pinv_mul_block: res is V, rectangular", b, pinv_mul_block, EINVAL_, a.res = v; a.ldr = mf);
  CASE("pinv_mul_block: last column of res inside jpvt", b, pinv_mul_block, EINVAL_, a.res = (double *)jpvt - 7 * nf);
  CASE("pinv_mul_block: V inside W2", bt, pinv_mul_block, EINVAL_, a.v = W2);
  CASE("pinv_mul_block: res inside the work space", b, pinv_mul_block, EINVAL_, a.res = work + 8 * (mf + nf) + 5);
  CASE("pinv_mul_block: k == 0 + null operand", b, pinv_mul_block, OK, a.k = 0; a.W2 = nullptr);
  CASE("pinv_mul_block: k == 0 + bad rank", b, pinv_mul_block, ESHAPE, a.k = 0; a.rank = nf);
  CASE("pinv_mul_block: negative nf + k == 0", b, pinv_mul_block, ESHAPE, a.nf = -7; a.k = 0);
  CASE("pinv_mul_block: bad rank + bad ldr", b, pinv_mul_block, ESHAPE, a.rank = 0; a.ldr = 1);
  CASE("pinv_mul_block: bad ldv + null operand", b, pinv_mul_block, ESHAPE, a.ldv = 1; a.v = nullptr);
  CASE("pinv_mul_block: null operand + overlap", b, pinv_mul_block, EINVAL_, a.jpvt = nullptr; a.res = W2);

  // ---- mxlo_getrf, mxlo_potrf, mxlo_ldlt (M may be NULL: the matrix is already in W)
  CASE("getrf: null ctx", s, getrf, EINVAL_, a.ctx = nullptr);
  CASE("getrf: complex dtype", s, getrf, EINVAL_, a.dtype = MXLO_C64);
  CASE("getrf: n < 0", s, getrf, ESHAPE, a.n = -1);
  CASE("getrf: ldw < n", s, getrf, ESHAPE, a.ldw = n - 1);
  CASE("getrf: null W", s, getrf, EINVAL_, a.W = nullptr);
  CASE("getrf: null info", s, getrf, EINVAL_, a.info = nullptr);
  CASE("getrf: n == 0 sets info 0", s, getrf, OK, a.n = 0; a.W = nullptr; a.dinv = nullptr);
  CASE("getrf: null perm", s, getrf, EINVAL_, a.jpvt = nullptr);
  CASE("getrf: null info word", s, getrf, EINVAL_, a.info_dev = nullptr);
  CASE("getrf: n too large", s, getrf, ESHAPE, a.n = a.ldw = a.ldm = 1LL << 31);
  CASE("getrf: ldm < n", s, getrf, ESHAPE, a.ldm = n - 1);
  CASE("getrf: W is M", s, getrf, EINVAL_, a.W = M);
  CASE("getrf: info word inside M", s, getrf, EINVAL_, a.info_dev = (int32_t *)(M + 3));
  CASE("getrf: perm's second 4 n bytes inside dinv_u", s, getrf, EINVAL_, a.dinv_u = (double *)jpvt + n / 2);
  CASE("getrf: dinv_u is dinv_l", s, getrf, EINVAL_, a.dinv_u = dinv);
  CASE("getrf: dinv_l inside W, no M", s, getrf, EINVAL_, a.M = nullptr; a.dinv = W + 9);
  ctx.capturing = true;
  CASE("getrf: during a capture", s, getrf, ESTATE, (void)a);
  CASE("getrf: overlap + capture", s, getrf, EINVAL_, a.W = M);
  ctx.capturing = false;
  CASE("getrf: bad dtype + bad shape", s, getrf, EINVAL_, a.dtype = 9; a.n = -1);
  CASE("getrf: bad shape + null info", s, getrf, ESHAPE, a.ldw = 1; a.info = nullptr);
  CASE("getrf: n == 0 + null info", s, getrf, EINVAL_, a.n = 0; a.info = nullptr);
  CASE("getrf: null storage + too large", s, getrf, EINVAL_, a.dinv = nullptr; a.n = a.ldw = a.ldm = 1LL << 31);
  CASE("getrf: bad ldm + overlap leaves info 0", s, getrf, ESHAPE, a.ldm = 1; a.dinv_u = dinv);
  CASE("potrf: null ctx", s, potrf, EINVAL_, a.ctx = nullptr);
  CASE("potrf: ldw < n", s, potrf, ESHAPE, a.ldw = n - 1);
  CASE("potrf: null info", s, potrf, EINVAL_, a.info = nullptr);
  CASE("potrf: n == 0 sets info 0", s, potrf, OK, a.n = 0; a.dinv = nullptr);
  CASE("potrf: null dinv", s, potrf, EINVAL_, a.dinv = nullptr);
  CASE("potrf: n too large", s, potrf, ESHAPE, a.n = a.ldw = a.ldm = 1LL << 31);
  CASE("potrf: ldm < n", s, potrf, ESHAPE, a.ldm = n - 1);
  CASE("potrf: W overlaps M, row-major", s, potrf, EINVAL_, a.rowmajor = 1; a.W = M + n * n - 1);
  CASE("potrf: null storage + bad ldm", s, potrf, EINVAL_, a.info_dev = nullptr; a.ldm = 1);
  CASE("potrf: bad ldm + overlap leaves info 0", s, potrf, ESHAPE, a.ldm = 1; a.W = M);
  ctx.capturing = true;
  CASE("potrf: during a capture, no M", s, potrf, ESTATE, a.M = nullptr);
  ctx.capturing = false;
  CASE("ldlt: null pivots", s, ldlt, EINVAL_, a.d = nullptr);
  CASE("ldlt: null pivots + null ctx", s, ldlt, EINVAL_, a.d = nullptr; a.ctx = nullptr);
  CASE("ldlt: null pivots + bad shape leaves info untouched", s, ldlt, EINVAL_, a.d = nullptr; a.ldw = 1);
  CASE("ldlt: n == 0, null pivots", s, ldlt, OK, a.n = 0; a.d = nullptr);
  CASE("ldlt: pivots inside W", s, ldlt, EINVAL_, a.d = W + 5);
  CASE("ldlt: pivots end inside dinv", s, ldlt, EINVAL_, a.d = dinv - n + 1);
  CASE("ldlt: too large + overlap", s, ldlt, ESHAPE, a.n = a.ldw = a.ldm = 1LL << 31; a.d = W);
  ctx.capturing = true;
  CASE("ldlt: overlap + capture", s, ldlt, EINVAL_, a.d = W);
  ctx.capturing = false;

  // ---- the square applies, one entry point per check path
  CASE("trisolve_mul: null ctx", s, trisolve_mul, EINVAL_, a.ctx = nullptr);
  CASE("trisolve_mul: complex dtype", s, trisolve_mul, EINVAL_, a.dtype = MXLO_C64);
  CASE("trisolve_mul: ld < n", s, trisolve_mul, ESHAPE, a.ldw = n - 1);
  CASE("trisolve_mul: null matrix", s, trisolve_mul, EINVAL_, a.W = nullptr);
  CASE("trisolve_mul: n == 0 launches nothing", s, trisolve_mul, OK, a.n = 0; a.res = nullptr; a.v = nullptr);
  CASE("trisolve_mul: n == 0 + bad op_mode", s, trisolve_mul, EINVAL_, a.n = 0; a.op = 77);
  CASE("trisolve_mul: null work", s, trisolve_mul, EINVAL_, a.work = nullptr);
  CASE("trisolve_mul: res is v", s, trisolve_mul, EINVAL_, a.res = v; a.op = 77);
  CASE("trisolve_mul: res overlaps v", s, trisolve_mul, EINVAL_, a.res = v + n - 1);
  CASE("trisolve_mul: v inside the block inverses", s, trisolve_mul, EINVAL_, a.v = dinv + 4 * 4096 - 1);
  CASE("trisolve_mul: res ends at the work vector's first double", s, trisolve_mul, EINVAL_, a.res = work - n + 1);
  CASE("trisolve_mul: bad op_mode", s, trisolve_mul, EINVAL_, a.op = 77);
  CASE("trisolve_mul: bad shape + null operand", s, trisolve_mul, ESHAPE, a.n = -1; a.res = nullptr);
  CASE("chol_mul_block: k == 0 launches nothing", s, chol_mul_block, OK, a.k = 0; a.res = nullptr; a.dinv = nullptr);
  CASE("chol_mul_block: k < 0", s, chol_mul_block, ESHAPE, a.k = -1);
  CASE("chol_mul_block: ldr < n", s, chol_mul_block, ESHAPE, a.ldr = n - 1);
  CASE("chol_mul_block: ldv < n", s, chol_mul_block, ESHAPE, a.ldv = n - 1);
  CASE("chol_mul_block: k == 0 + bad ldv", s, chol_mul_block, ESHAPE, a.k = 0; a.ldv = 0);
  CASE("chol_mul_block: n == 0 + ld 0", s, chol_mul_block, ESHAPE, a.n = 0; a.ldw = 0);
  CASE("chol_mul_block: null V", s, chol_mul_block, EINVAL_, a.v = nullptr);
  CASE("chol_mul_block: res is V in another leading dimension", s, chol_mul_block, EINVAL_, a.res = v; a.ldr = n + 1; a.k = 7);
  CASE("chol_mul_block: last column of res inside L", s, chol_mul_block, EINVAL_, a.res = W - 7 * n);
  CASE("chol_mul_block: V inside the work matrix's eighth column", s, chol_mul_block, EINVAL_, a.v = work + 8 * n - 1);
  CASE("chol_mul_block: bad k + null matrix", s, chol_mul_block, EINVAL_, a.k = -1; a.W = nullptr);
  CASE("chol_mul_block: bad ldr + null operand", s, chol_mul_block, ESHAPE, a.ldr = 1; a.work = nullptr);
  CASE("ldl_mul: n == 0, null pivots", s, ldl_mul, OK, a.n = 0; a.d = nullptr);
  CASE("ldl_mul: null pivots", s, ldl_mul, EINVAL_, a.d = nullptr);
  CASE("ldl_mul: res inside the pivots", s, ldl_mul, EINVAL_, a.res = b.d + n - 1);
  CASE("ldl_mul: v inside the pivots, float", s, ldl_mul, EINVAL_, a.dtype = F32; a.v = (double *)((float *)b.d - n + 1));
  CASE("ldl_mul: bad shape + null pivots", s, ldl_mul, ESHAPE, a.ldw = 1; a.d = nullptr);
  CASE("ldl_mul_block: k == 0, null pivots", s, ldl_mul_block, OK, a.k = 0; a.d = nullptr);
  CASE("ldl_mul_block: null pivots", s, ldl_mul_block, EINVAL_, a.d = nullptr);
  CASE("ldl_mul_block: last column of V inside the pivots", s, ldl_mul_block, EINVAL_, a.v = b.d - 7 * n);
  CASE("ldl_mul_block: bad ldv + null pivots", s, ldl_mul_block, ESHAPE, a.ldv = 1; a.d = nullptr);
  CASE("lu_mul: null second block inverses", s, lu_mul, EINVAL_, a.dinv_u = nullptr);
  CASE("lu_mul: res inside the permutation", s, lu_mul, EINVAL_, a.res = (double *)jpvt + n / 2 - 1);
  CASE("lu_mul: n == 0 + bad op_mode", s, lu_mul, EINVAL_, a.n = 0; a.op = 77);
  CASE("lu_mul: n == 0, null operands", s, lu_mul, OK, a.n = 0; a.W = nullptr; a.jpvt = nullptr);
  CASE("lu_mul_block: null permutation", s, lu_mul_block, EINVAL_, a.jpvt = nullptr);
  CASE("lu_mul_block: k == 0 + bad op_mode", s, lu_mul_block, EINVAL_, a.k = 0; a.op = 77);
  CASE("lu_mul_block: k == 0, null operands", s, lu_mul_block, OK, a.k = 0; a.dinv_u = nullptr; a.jpvt = nullptr);
  CASE("lu_mul_block: V inside the second block inverses", s, lu_mul_block, EINVAL_, a.v = b.dinv_u + 4 * 4096 - 1);
  CASE("lu_mul_block: res is V", s, lu_mul_block, EINVAL_, a.res = v; a.op = 77);
  CASE("lu_mul_block: bad ldr + null permutation", s, lu_mul_block, ESHAPE, a.ldr = 1; a.jpvt = nullptr);
  CASE("lu_mul_block: null permutation + bad op_mode", s, lu_mul_block, EINVAL_, a.jpvt = nullptr; a.op = 77);
  CASE("ldl_mul_refine: steps > 8", s, ldl_mul_refine, EINVAL_, a.steps = 9);
  CASE("ldl_mul_refine: k == 0 + steps < 0", s, ldl_mul_refine, EINVAL_, a.k = 0; a.steps = -1);
  CASE("ldl_mul_refine: k == 0, null operands", s, ldl_mul_refine, OK, a.k = 0; a.d = nullptr; a.dg = nullptr);
  CASE("ldl_mul_refine: null pivots", s, ldl_mul_refine, EINVAL_, a.d = nullptr);
  CASE("ldl_mul_refine: null diagonal", s, ldl_mul_refine, EINVAL_, a.dg = nullptr);
  CASE("ldl_mul_refine: res inside the diagonal", s, ldl_mul_refine, EINVAL_, a.res = b.dg + n - 1);
  CASE("ldl_mul_refine: res inside the second work matrix", s, ldl_mul_refine, EINVAL_, a.res = work + 16 * n - 1);
  CASE("ldl_mul_refine: bad ldr + bad steps", s, ldl_mul_refine, ESHAPE, a.ldr = 1; a.steps = 9);
  CASE("lu_mul_refine: lda < n", s, lu_mul_refine, ESHAPE, a.lda = n - 1);
  CASE("lu_mul_refine: k == 0 + lda < n", s, lu_mul_refine, ESHAPE, a.k = 0; a.lda = 0);
  CASE("lu_mul_refine: bad op_mode + lda < n", s, lu_mul_refine, EINVAL_, a.op = 77; a.lda = 1);
  CASE("lu_mul_refine: overlap + lda < n", s, lu_mul_refine, EINVAL_, a.res = W; a.lda = 1);
  CASE("lu_mul_refine: lda < n + steps > 8", s, lu_mul_refine, ESHAPE, a.lda = 1; a.steps = 9);
  CASE("lu_mul_refine: lda < n + res inside the second work matrix", s, lu_mul_refine, ESHAPE, a.lda = 1; a.res = work + 16 * n - 1);
  CASE("lu_mul_refine: lda < n + null snapshot", s, lu_mul_refine, ESHAPE, a.lda = 1; a.A2 = nullptr);
  CASE("lu_mul_refine: null snapshot", s, lu_mul_refine, EINVAL_, a.A2 = nullptr);
  CASE("lu_mul_refine: V inside the snapshot", s, lu_mul_refine, EINVAL_, a.v = b.A2 + n * n - 1);
  CASE("lu_mul_refine: k == 0, null operands", s, lu_mul_refine, OK, a.k = 0; a.A2 = nullptr; a.jpvt = nullptr);

  // ---- mxlo_sytrf and its applies
  const Args y = s;
  CASE("sytrf: null ctx", y, sytrf, EINVAL_, a.ctx = nullptr);
  CASE("sytrf: complex dtype", y, sytrf, EINVAL_, a.dtype = MXLO_C64);
  CASE("sytrf: n < 0", y, sytrf, ESHAPE, a.n = -1);
  CASE("sytrf: ldw < n", y, sytrf, ESHAPE, a.ldw = n - 1);
  CASE("sytrf: null W", y, sytrf, EINVAL_, a.W = nullptr);
  CASE("sytrf: null info", y, sytrf, EINVAL_, a.info = nullptr);
  CASE("sytrf: n == 0 sets info 0", y, sytrf, OK, a.n = 0; a.W = nullptr; a.d = nullptr; a.e = nullptr; a.perm = nullptr);
  CASE("sytrf: null block inverses", y, sytrf, EINVAL_, a.dinv = nullptr);
  CASE("sytrf: null d", y, sytrf, EINVAL_, a.d = nullptr);
  CASE("sytrf: null e", y, sytrf, EINVAL_, a.e = nullptr);
  CASE("sytrf: null perm", y, sytrf, EINVAL_, a.perm = nullptr);
  CASE("sytrf: null panel workspace", y, sytrf, EINVAL_, a.panel = nullptr);
  CASE("sytrf: null info word", y, sytrf, EINVAL_, a.info_dev = nullptr);
  CASE("sytrf: n too large", y, sytrf, ESHAPE, a.n = a.ldw = a.ldm = 1LL << 31);
  CASE("sytrf: ldm < n", y, sytrf, ESHAPE, a.ldm = n - 1);
  CASE("sytrf: no M, factored in place", y, sytrf, EINVAL_, a.M = nullptr; a.e = W);
  CASE("sytrf: W is M", y, sytrf, EINVAL_, a.W = M);
  CASE("sytrf: W overlaps M, row-major", y, sytrf, EINVAL_, a.rowmajor = 1; a.W = M + n * n - 1);
  CASE("sytrf: d inside W", y, sytrf, EINVAL_, a.d = W + 5);
  CASE("sytrf: e ends inside the block inverses", y, sytrf, EINVAL_, a.e = dinv - n + 1);
  CASE("sytrf: e is d", y, sytrf, EINVAL_, a.e = y.d);
  CASE("sytrf: perm's panel starts inside d", y, sytrf, EINVAL_, a.perm = (int32_t *)y.d - 2 * n - 1);
  CASE("sytrf: perm inside W", y, sytrf, EINVAL_, a.perm = (int32_t *)(W + 9));
  CASE("sytrf: panel workspace's last element inside W, no M", y, sytrf, EINVAL_, a.M = nullptr; a.panel = W - 65 * n + 1);
  CASE("sytrf: panel workspace inside M", y, sytrf, EINVAL_, a.panel = M + 3);
  CASE("sytrf: info word inside M", y, sytrf, EINVAL_, a.info_dev = (int32_t *)(M + 3));
  ctx.capturing = true;
  CASE("sytrf: during a capture", y, sytrf, ESTATE, (void)a);
  CASE("sytrf: during a capture, float, no M", y, sytrf, ESTATE, a.dtype = F32; a.M = nullptr);
  CASE("sytrf: overlap + capture", y, sytrf, EINVAL_, a.d = W);
  ctx.capturing = false;
  CASE("sytrf: bad dtype + bad shape", y, sytrf, EINVAL_, a.dtype = 9; a.n = -1);
  CASE("sytrf: bad shape + null info", y, sytrf, ESHAPE, a.ldw = 1; a.info = nullptr);
  CASE("sytrf: null storage + too large", y, sytrf, EINVAL_, a.e = nullptr; a.n = a.ldw = a.ldm = 1LL << 31);
  CASE("sytrf: bad ldm + overlap leaves info 0", y, sytrf, ESHAPE, a.ldm = 1; a.e = y.d);
  CASE("ldlp_mul: null ctx", y, ldlp_mul, EINVAL_, a.ctx = nullptr);
  CASE("ldlp_mul: complex dtype", y, ldlp_mul, EINVAL_, a.dtype = MXLO_C64);
  CASE("ldlp_mul: ld < n", y, ldlp_mul, ESHAPE, a.ldw = n - 1);
  CASE("ldlp_mul: n == 0, null operands", y, ldlp_mul, OK, a.n = 0; a.d = nullptr; a.e = nullptr; a.perm = nullptr);
  CASE("ldlp_mul: null res", y, ldlp_mul, EINVAL_, a.res = nullptr);
  CASE("ldlp_mul: null d", y, ldlp_mul, EINVAL_, a.d = nullptr);
  CASE("ldlp_mul: null e", y, ldlp_mul, EINVAL_, a.e = nullptr);
  CASE("ldlp_mul: null perm", y, ldlp_mul, EINVAL_, a.perm = nullptr);
  CASE("ldlp_mul: null work", y, ldlp_mul, EINVAL_, a.work = nullptr);
  CASE("ldlp_mul: res overlaps v", y, ldlp_mul, EINVAL_, a.res = v + n - 1);
  CASE("ldlp_mul: res inside e", y, ldlp_mul, EINVAL_, a.res = y.e + n - 1);
  CASE("ldlp_mul: v inside d, float", y, ldlp_mul, EINVAL_, a.dtype = F32; a.v = (double *)((float *)y.d - n + 1));
  CASE("ldlp_mul: res ends at the permutation's first word", y, ldlp_mul, EINVAL_, a.res = (double *)y.perm - n + 1);
  CASE("ldlp_mul: res behind the permutation's n words", y, ldlp_mul, EINVAL_, a.res = (double *)y.perm + n / 2 - 1);
  CASE("ldlp_mul: bad shape + null e", y, ldlp_mul, ESHAPE, a.ldw = 1; a.e = nullptr);
  CASE("ldlp_mul_block: k == 0, null operands", y, ldlp_mul_block, OK, a.k = 0; a.d = nullptr; a.e = nullptr; a.perm = nullptr);
  CASE("ldlp_mul_block: k < 0", y, ldlp_mul_block, ESHAPE, a.k = -1);
  CASE("ldlp_mul_block: ldr < n", y, ldlp_mul_block, ESHAPE, a.ldr = n - 1);
  CASE("ldlp_mul_block: ldv < n", y, ldlp_mul_block, ESHAPE, a.ldv = n - 1);
  CASE("ldlp_mul_block: null e", y, ldlp_mul_block, EINVAL_, a.e = nullptr);
  CASE("ldlp_mul_block: null perm", y, ldlp_mul_block, EINVAL_, a.perm = nullptr);
  CASE("ldlp_mul_block: res is V in another leading dimension", y, ldlp_mul_block, EINVAL_, a.res = v; a.ldr = n + 1; a.k = 7);
  CASE("ldlp_mul_block: last column of V inside e", y, ldlp_mul_block, EINVAL_, a.v = y.e - 7 * n);
  CASE("ldlp_mul_block: last column of res inside L", y, ldlp_mul_block, EINVAL_, a.res = W - 7 * n);
  CASE("ldlp_mul_block: V inside the work matrix's eighth column", y, ldlp_mul_block, EINVAL_, a.v = work + 8 * n - 1);
  CASE("ldlp_mul_block: bad ldv + null perm", y, ldlp_mul_block, ESHAPE, a.ldv = 1; a.perm = nullptr);

  // ---- the snapshots and the residuals of the refined applies
  CASE("sym_snapshot: null ctx", s, sym_snapshot, EINVAL_, a.ctx = nullptr);
  CASE("sym_snapshot: complex dtype", s, sym_snapshot, EINVAL_, a.dtype = MXLO_C64);
  CASE("sym_snapshot: ldw < n", s, sym_snapshot, ESHAPE, a.ldw = n - 1);
  CASE("sym_snapshot: null W", s, sym_snapshot, EINVAL_, a.W = nullptr);
  CASE("sym_snapshot: n == 0 launches nothing", s, sym_snapshot, OK, a.n = 0; a.M = nullptr; a.W = nullptr; a.dg = nullptr);
  CASE("sym_snapshot: null M", s, sym_snapshot, EINVAL_, a.M = nullptr);
  CASE("sym_snapshot: null diagonal", s, sym_snapshot, EINVAL_, a.dg = nullptr);
  CASE("sym_snapshot: ldm one too small", s, sym_snapshot, EINVAL_, a.ldm = n - 1);
  CASE("sym_snapshot: n too large", s, sym_snapshot, ESHAPE, a.n = a.ldw = a.ldm = 1LL << 31);
  CASE("sym_snapshot: W is M", s, sym_snapshot, EINVAL_, a.W = M);
  CASE("sym_snapshot: W starts at the last element of M, row-major", s, sym_snapshot, EINVAL_, a.rowmajor = 1; a.W = M + n * n - 1);
  CASE("sym_snapshot: diagonal inside M", s, sym_snapshot, EINVAL_, a.dg = M + 7);
  CASE("sym_snapshot: diagonal ends at the first element of W", s, sym_snapshot, EINVAL_, a.dg = W - n + 1);
  CASE("sym_snapshot: diagonal inside W, float", s, sym_snapshot, EINVAL_, a.dtype = F32; a.dg = (double *)((float *)W + n * n - 1));
  CASE("sym_snapshot: bad ldw + null M", s, sym_snapshot, ESHAPE, a.ldw = 1; a.M = nullptr);
  CASE("sym_snapshot: short ldm + overlap", s, sym_snapshot, EINVAL_, a.ldm = 1; a.W = M);
  CASE("sym_snapshot: null diagonal + too large", s, sym_snapshot, EINVAL_, a.dg = nullptr; a.n = a.ldw = a.ldm = 1LL << 31);
  CASE("sym_snapshot: too large + overlap", s, sym_snapshot, ESHAPE, a.n = a.ldw = a.ldm = 1LL << 31; a.W = M);
  CASE("lu_snapshot: null ctx", s, lu_snapshot, EINVAL_, a.ctx = nullptr);
  CASE("lu_snapshot: complex dtype", s, lu_snapshot, EINVAL_, a.dtype = MXLO_C32);
  CASE("lu_snapshot: lda < n", s, lu_snapshot, ESHAPE, a.lda = n - 1);
  CASE("lu_snapshot: null snapshot", s, lu_snapshot, EINVAL_, a.A2 = nullptr);
  CASE("lu_snapshot: n == 0 launches nothing", s, lu_snapshot, OK, a.n = 0; a.M = nullptr; a.A2 = nullptr; a.jpvt = nullptr);
  CASE("lu_snapshot: null M", s, lu_snapshot, EINVAL_, a.M = nullptr);
  CASE("lu_snapshot: null permutation", s, lu_snapshot, EINVAL_, a.jpvt = nullptr);
  CASE("lu_snapshot: ldm one too small", s, lu_snapshot, EINVAL_, a.ldm = n - 1);
  CASE("lu_snapshot: n too large", s, lu_snapshot, ESHAPE, a.n = a.lda = a.ldm = 1LL << 31);
  CASE("lu_snapshot: snapshot is M", s, lu_snapshot, EINVAL_, a.A2 = M);
  CASE("lu_snapshot: snapshot ends at the first element of M", s, lu_snapshot, EINVAL_, a.A2 = M - n * n + 1);
  CASE("lu_snapshot: permutation inside the snapshot", s, lu_snapshot, EINVAL_, a.jpvt = (int32_t *)(s.A2 + 9));
  CASE("lu_snapshot: permutation's last word inside the snapshot", s, lu_snapshot, EINVAL_, a.jpvt = (int32_t *)s.A2 - n + 1);
  CASE("lu_snapshot: bad lda + null M", s, lu_snapshot, ESHAPE, a.lda = 1; a.M = nullptr);
  CASE("lu_snapshot: short ldm + overlap", s, lu_snapshot, EINVAL_, a.ldm = 1; a.A2 = M);
  CASE("lu_snapshot: null permutation + too large", s, lu_snapshot, EINVAL_, a.jpvt = nullptr; a.n = a.lda = a.ldm = 1LL << 31);
  CASE("lu_snapshot: too large + overlap", s, lu_snapshot, ESHAPE, a.n = a.lda = a.ldm = 1LL << 31; a.A2 = M);
  CASE("sym_residual: null ctx", s, sym_residual, EINVAL_, a.ctx = nullptr);
  CASE("sym_residual: complex dtype", s, sym_residual, EINVAL_, a.dtype = MXLO_C64);
  CASE("sym_residual: ld < n", s, sym_residual, ESHAPE, a.ldw = n - 1);
  CASE("sym_residual: null matrix", s, sym_residual, EINVAL_, a.W = nullptr);
  CASE("sym_residual: k < 0", s, sym_residual, ESHAPE, a.k = -1);
  CASE("sym_residual: k == 9", s, sym_residual, ESHAPE, a.k = 9);
  CASE("sym_residual: ldv one too small", s, sym_residual, ESHAPE, a.ldv = n - 1);
  CASE("sym_residual: n == 0 launches nothing", s, sym_residual, OK, a.n = 0; a.R = nullptr; a.X = nullptr; a.v = nullptr; a.dg = nullptr);
  CASE("sym_residual: k == 0 launches nothing", s, sym_residual, OK, a.k = 0; a.R = nullptr; a.X = nullptr; a.v = nullptr; a.dg = nullptr);
  CASE("sym_residual: null R", s, sym_residual, EINVAL_, a.R = nullptr);
  CASE("sym_residual: null V", s, sym_residual, EINVAL_, a.v = nullptr);
  CASE("sym_residual: null X", s, sym_residual, EINVAL_, a.X = nullptr);
  CASE("sym_residual: null diagonal", s, sym_residual, EINVAL_, a.dg = nullptr);
  CASE("sym_residual: n too large", s, sym_residual, ESHAPE, a.n = a.ldw = a.ldv = 1LL << 31);
  CASE("sym_residual: R is X", s, sym_residual, EINVAL_, a.R = s.X);
  CASE("sym_residual: R ends at the first double of X", s, sym_residual, EINVAL_, a.R = s.X - 8 * n + 1);
  CASE("sym_residual: R inside the last column of V", s, sym_residual, EINVAL_, a.R = v + 8 * n - 1);
  CASE("sym_residual: R inside the matrix", s, sym_residual, EINVAL_, a.R = W + n * n - 1);
  CASE("sym_residual: R inside the diagonal", s, sym_residual, EINVAL_, a.R = s.dg + n - 1);
  CASE("sym_residual: X is V, which is allowed, + null diagonal", s, sym_residual, EINVAL_, a.X = v; a.dg = nullptr);
  CASE("sym_residual: bad k + null matrix", s, sym_residual, EINVAL_, a.k = 9; a.W = nullptr);
  CASE("sym_residual: short ldv + null R", s, sym_residual, ESHAPE, a.ldv = 1; a.R = nullptr);
  CASE("sym_residual: null X + too large", s, sym_residual, EINVAL_, a.X = nullptr; a.n = a.ldw = a.ldv = 1LL << 31);
  CASE("sym_residual: too large + overlap", s, sym_residual, ESHAPE, a.n = a.ldw = a.ldv = 1LL << 31; a.R = s.X);
  CASE("sym_residual: overlap + null diagonal", s, sym_residual, EINVAL_, a.R = s.X; a.dg = nullptr);
  CASE("gen_residual: null ctx", s, gen_residual, EINVAL_, a.ctx = nullptr);
  CASE("gen_residual: lda < n", s, gen_residual, ESHAPE, a.lda = n - 1);
  CASE("gen_residual: k == 9", s, gen_residual, ESHAPE, a.k = 9);
  CASE("gen_residual: ldv one too small", s, gen_residual, ESHAPE, a.ldv = n - 1);
  CASE("gen_residual: bad op_mode", s, gen_residual, EINVAL_, a.op = 77);
  CASE("gen_residual: n == 0 launches nothing", s, gen_residual, OK, a.n = 0; a.R = nullptr; a.X = nullptr; a.v = nullptr; a.A2 = nullptr);
  CASE("gen_residual: k == 0 launches nothing, transposed", s, gen_residual, OK, a.k = 0; a.op = T; a.R = nullptr);
  CASE("gen_residual: k == 0 + bad op_mode", s, gen_residual, EINVAL_, a.k = 0; a.op = 77);
  CASE("gen_residual: null R", s, gen_residual, EINVAL_, a.R = nullptr);
  CASE("gen_residual: null V", s, gen_residual, EINVAL_, a.v = nullptr);
  CASE("gen_residual: R is X", s, gen_residual, EINVAL_, a.R = s.X);
  CASE("gen_residual: R ends at the first element of V", s, gen_residual, EINVAL_, a.R = v - 8 * n + 1);
  CASE("gen_residual: R inside the matrix, float", s, gen_residual, EINVAL_, a.dtype = F32; a.R = (double *)((float *)s.A2 + n * n - 1));
  CASE("gen_residual: short ldv + bad op_mode", s, gen_residual, ESHAPE, a.ldv = 1; a.op = 77);
  CASE("gen_residual: overlap + bad op_mode", s, gen_residual, EINVAL_, a.R = s.X; a.op = 77);
  CASE("gen_residual: too large + bad op_mode", s, gen_residual, ESHAPE, a.n = a.lda = a.ldv = 1LL << 31; a.op = 77);

  // ---- both members of each vector / block pair, the same cases
  pair_cases("trisolve_mul", s, trisolve_mul, false, true);
  pair_cases("trisolve_mul_block", s, trisolve_mul_block, true, true);
  pair_cases("chol_mul", s, chol_mul, false, true);
  pair_cases("chol_mul_block", s, chol_mul_block, true, true);
  pair_cases("ldl_mul", s, ldl_mul, false, true);
  pair_cases("ldl_mul_block", s, ldl_mul_block, true, true);
  pair_cases("lu_mul", s, lu_mul, false, true);
  pair_cases("lu_mul_block", s, lu_mul_block, true, true);
  pair_cases("ldlp_mul", s, ldlp_mul, false, true);
  pair_cases("ldlp_mul_block", s, ldlp_mul_block, true, true);
  pair_cases("qr_mul", b, qr_mul, false, false);
  pair_cases("qr_mul_block", b, qr_mul_block, true, false);
  pair_cases("qrp_mul", b, qrp_mul, false, false);
  pair_cases("qrp_mul_block", b, qrp_mul_block, true, false);
  pair_cases("pinv_mul", b, pinv_mul, false, false);
  pair_cases("pinv_mul_block", b, pinv_mul_block, true, false);
  pair_cases("lu_mul, transposed", [&] { Args a = s; a.op = T; return a; }(), lu_mul, false, true);
  pair_cases("lu_mul_block, transposed", [&] { Args a = s; a.op = T; return a; }(), lu_mul_block, true, true);

  std::printf("%d calls, %d unexpected\n", lines, failures);
  return failures ? 1 : 0;
}
