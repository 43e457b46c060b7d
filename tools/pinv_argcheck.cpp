// Host-side memory check of the argument checks of mxlo_cod_factor, mxlo_pinv_mul and mxlo_pinv_mul_block: every call below must
// be refused (null operands, bad shapes, a bad rank, overlaps) before anything touches a device, so the program needs no GPU.
// The pointers are addresses inside one host buffer that is never dereferenced by the library. Build the host code with
// AddressSanitizer and UBSan and run it (from the repository root):
//
//   hipcc -O1 -g -std=c++20 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Iinclude tools/pinv_argcheck.cpp linearoperators.jl_amd/csrc/linalg.hip linearoperators.jl_amd/csrc/api_ctx.hip \
//       -o /tmp/pinv_argcheck && /tmp/pinv_argcheck
//
// It prints one line per refusal and exits 0 when every status is the expected one.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../linearoperators.jl_amd/csrc/common.h"
#include "mxlo.h"

namespace mxlo {                                        // api_ctx.hip (mxlo_last_error) refers to it; the quasi-Newton code is not linked
bool qn_generation(const mxlo_qn *, int64_t *) { return false; }
}

static int failures = 0;

static void expect(const char *what, int32_t got, int32_t want) {
  std::printf("%-58s status %d (%s)%s\n", what, got, got ? mxlo_last_error() : "ok", got == want ? "" : "   <-- UNEXPECTED");
  if (got != want) ++failures;
}

int main() {
  mxlo_ctx ctx;                                         // never used for a launch: every call returns before the device guard
  const int64_t mf = 200, nf = 129, r = 65, nb = 2, scratch_len = 2 * (512 * 64 + 64) + (512 + 2 * nb) * 4096;
  std::vector<double> pool(8 * (mf + nf + 2 * 512 * 64) + mf * nf + nf * r + 3 * nb * 4096 + nf + scratch_len + 16 * mf + 4096);
  double *p = pool.data();
  double *W = p; p += mf * nf;
  double *tfac = p; p += nb * 4096;
  int32_t *jpvt = (int32_t *)p; p += nf;
  double *W2 = p; p += nf * r;
  double *tfac2 = p; p += nb * 4096;
  double *dinv2 = p; p += nb * 4096;
  double *scratch = p; p += scratch_len;
  int32_t *info_dev = (int32_t *)p; p += 1;
  double *work = p; p += 8 * (mf + nf + 2 * 512 * 64);
  double *res = p; p += 8 * mf;
  double *v = p; p += 8 * mf;
  int32_t info = -1;
  const int32_t F64 = MXLO_F64, N = MXLO_OP_N, T = MXLO_OP_T;

  // ---- mxlo_cod_factor
  expect("cod_factor: null ctx", mxlo_cod_factor(nullptr, F64, W, mf, nf, r, W2, tfac2, dinv2, scratch, scratch_len, info_dev, &info), MXLO_EINVAL);
  expect("cod_factor: complex dtype", mxlo_cod_factor(&ctx, MXLO_C64, W, mf, nf, r, W2, tfac2, dinv2, scratch, scratch_len, info_dev, &info), MXLO_EINVAL);
  expect("cod_factor: nf == 0", mxlo_cod_factor(&ctx, F64, W, mf, 0, r, W2, tfac2, dinv2, scratch, scratch_len, info_dev, &info), MXLO_ESHAPE);
  expect("cod_factor: ldw < nf", mxlo_cod_factor(&ctx, F64, W, nf - 1, nf, r, W2, tfac2, dinv2, scratch, scratch_len, info_dev, &info), MXLO_ESHAPE);
  expect("cod_factor: nf too large", mxlo_cod_factor(&ctx, F64, W, 1LL << 31, 1LL << 31, r, W2, tfac2, dinv2, scratch, scratch_len, info_dev, &info), MXLO_ESHAPE);
  expect("cod_factor: rank 0", mxlo_cod_factor(&ctx, F64, W, mf, nf, 0, W2, tfac2, dinv2, scratch, scratch_len, info_dev, &info), MXLO_ESHAPE);
  expect("cod_factor: rank > nf", mxlo_cod_factor(&ctx, F64, W, mf, nf, nf + 1, W2, tfac2, dinv2, scratch, scratch_len, info_dev, &info), MXLO_ESHAPE);
  expect("cod_factor: null W", mxlo_cod_factor(&ctx, F64, nullptr, mf, nf, r, W2, tfac2, dinv2, scratch, scratch_len, info_dev, &info), MXLO_EINVAL);
  expect("cod_factor: null W2", mxlo_cod_factor(&ctx, F64, W, mf, nf, r, nullptr, tfac2, dinv2, scratch, scratch_len, info_dev, &info), MXLO_EINVAL);
  expect("cod_factor: null dinv2", mxlo_cod_factor(&ctx, F64, W, mf, nf, r, W2, tfac2, nullptr, scratch, scratch_len, info_dev, &info), MXLO_EINVAL);
  expect("cod_factor: null info", mxlo_cod_factor(&ctx, F64, W, mf, nf, r, W2, tfac2, dinv2, scratch, scratch_len, info_dev, nullptr), MXLO_EINVAL);
  expect("cod_factor: scratch too short", mxlo_cod_factor(&ctx, F64, W, mf, nf, r, W2, tfac2, dinv2, scratch, scratch_len - 1, info_dev, &info), MXLO_ESHAPE);
  expect("cod_factor: W2 is W", mxlo_cod_factor(&ctx, F64, W, mf, nf, r, W, tfac2, dinv2, scratch, scratch_len, info_dev, &info), MXLO_EINVAL);
  expect("cod_factor: W2 starts in the last column of W", mxlo_cod_factor(&ctx, F64, W, mf, nf, r, W + (nf - 1) * mf + r - 1, tfac2, dinv2, scratch, scratch_len, info_dev, &info), MXLO_EINVAL);
  expect("cod_factor: tfac2 inside W2", mxlo_cod_factor(&ctx, F64, W, mf, nf, r, W2, W2 + 7, dinv2, scratch, scratch_len, info_dev, &info), MXLO_EINVAL);
  expect("cod_factor: dinv2 is tfac2", mxlo_cod_factor(&ctx, F64, W, mf, nf, r, W2, tfac2, tfac2, scratch, scratch_len, info_dev, &info), MXLO_EINVAL);
  expect("cod_factor: info word inside the scratch", mxlo_cod_factor(&ctx, F64, W, mf, nf, r, W2, tfac2, dinv2, scratch, scratch_len, (int32_t *)scratch + 5, &info), MXLO_EINVAL);
  ctx.capturing = true;
  expect("cod_factor: during a capture", mxlo_cod_factor(&ctx, F64, W, mf, nf, r, W2, tfac2, dinv2, scratch, scratch_len, info_dev, &info), MXLO_ESTATE);
  ctx.capturing = false;

  // ---- mxlo_pinv_mul
  expect("pinv_mul: null ctx", mxlo_pinv_mul(nullptr, F64, res, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, v, N, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul: complex dtype", mxlo_pinv_mul(&ctx, MXLO_C64, res, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, v, N, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul: bad op_mode", mxlo_pinv_mul(&ctx, F64, res, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, v, 77, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul: nf > mf", mxlo_pinv_mul(&ctx, F64, res, W, mf, nf, mf, tfac, jpvt, r, W2, tfac2, dinv2, work, v, N, 1.0, 0.0), MXLO_ESHAPE);
  expect("pinv_mul: ldw < mf", mxlo_pinv_mul(&ctx, F64, res, W, mf - 1, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, v, N, 1.0, 0.0), MXLO_ESHAPE);
  expect("pinv_mul: rank 0", mxlo_pinv_mul(&ctx, F64, res, W, mf, mf, nf, tfac, jpvt, 0, W2, tfac2, dinv2, work, v, N, 1.0, 0.0), MXLO_ESHAPE);
  expect("pinv_mul: rank == nf", mxlo_pinv_mul(&ctx, F64, res, W, mf, mf, nf, tfac, jpvt, nf, W2, tfac2, dinv2, work, v, N, 1.0, 0.0), MXLO_ESHAPE);
  expect("pinv_mul: null jpvt", mxlo_pinv_mul(&ctx, F64, res, W, mf, mf, nf, tfac, nullptr, r, W2, tfac2, dinv2, work, v, N, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul: null W2", mxlo_pinv_mul(&ctx, F64, res, W, mf, mf, nf, tfac, jpvt, r, nullptr, tfac2, dinv2, work, v, N, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul: null dinv2", mxlo_pinv_mul(&ctx, F64, res, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, nullptr, work, v, N, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul: null res", mxlo_pinv_mul(&ctx, F64, nullptr, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, v, N, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul: res is v, rectangular", mxlo_pinv_mul(&ctx, F64, v, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, v, N, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul: res overlaps v", mxlo_pinv_mul(&ctx, F64, v + 1, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, v, T, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul: res inside jpvt", mxlo_pinv_mul(&ctx, F64, (double *)jpvt, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, v, N, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul: res inside W2", mxlo_pinv_mul(&ctx, F64, W2 + nf * r - 1, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, v, N, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul: v inside dinv2", mxlo_pinv_mul(&ctx, F64, res, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, dinv2 + 9, N, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul: v ends inside tfac2", mxlo_pinv_mul(&ctx, F64, res, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, tfac2 - mf + 1, N, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul: res inside the work vector", mxlo_pinv_mul(&ctx, F64, work + mf + 2 * 512 * 64 - 1, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, v, N, 1.0, 0.0), MXLO_EINVAL);

  // ---- mxlo_pinv_mul_block
  expect("pinv_mul_block: null ctx", mxlo_pinv_mul_block(nullptr, F64, res, nf, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, v, mf, 8, N, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul_block: k == 0 launches nothing", mxlo_pinv_mul_block(&ctx, F64, nullptr, nf, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, nullptr, mf, 0, N, 1.0, 0.0), MXLO_OK);
  expect("pinv_mul_block: k < 0", mxlo_pinv_mul_block(&ctx, F64, res, nf, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, v, mf, -1, N, 1.0, 0.0), MXLO_ESHAPE);
  expect("pinv_mul_block: ldr < nf", mxlo_pinv_mul_block(&ctx, F64, res, nf - 1, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, v, mf, 8, N, 1.0, 0.0), MXLO_ESHAPE);
  expect("pinv_mul_block: ldv < nf, transposed", mxlo_pinv_mul_block(&ctx, F64, res, mf, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, v, nf - 1, 8, T, 1.0, 0.0), MXLO_ESHAPE);
  expect("pinv_mul_block: rank == nf", mxlo_pinv_mul_block(&ctx, F64, res, nf, W, mf, mf, nf, tfac, jpvt, nf, W2, tfac2, dinv2, work, v, mf, 8, N, 1.0, 0.0), MXLO_ESHAPE);
  expect("pinv_mul_block: rank < 1", mxlo_pinv_mul_block(&ctx, F64, res, nf, W, mf, mf, nf, tfac, jpvt, -3, W2, tfac2, dinv2, work, v, mf, 8, N, 1.0, 0.0), MXLO_ESHAPE);
  expect("pinv_mul_block: null tfac2", mxlo_pinv_mul_block(&ctx, F64, res, nf, W, mf, mf, nf, tfac, jpvt, r, W2, nullptr, dinv2, work, v, mf, 8, N, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul_block: null V", mxlo_pinv_mul_block(&ctx, F64, res, nf, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, nullptr, mf, 8, N, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul_block: res is V, rectangular", mxlo_pinv_mul_block(&ctx, F64, v, mf, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, v, mf, 8, N, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul_block: last column of res inside jpvt", mxlo_pinv_mul_block(&ctx, F64, (double *)jpvt - 7 * nf, nf, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, v, mf, 8, N, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul_block: V inside W2", mxlo_pinv_mul_block(&ctx, F64, res, mf, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, W2, nf, 8, T, 1.0, 0.0), MXLO_EINVAL);
  expect("pinv_mul_block: res inside the work space", mxlo_pinv_mul_block(&ctx, F64, work + 8 * (mf + nf) + 5, nf, W, mf, mf, nf, tfac, jpvt, r, W2, tfac2, dinv2, work, v, mf, 8, N, 1.0, 0.0), MXLO_EINVAL);

  std::printf("%d unexpected\n", failures);
  return failures ? 1 : 0;
}
