// Host-side memory check of the argument checks of mxlo_geqp3, mxlo_qrp_mul and mxlo_qrp_mul_block: every call below must be
// refused (null operands, bad shapes, overlaps, a bad rank or rtol) before anything touches a device, so the program needs no
// GPU. The pointers are addresses inside one host buffer that is never dereferenced by the library. Build the host code with
// AddressSanitizer and UBSan and run it (from the repository root):
//
//   hipcc -O1 -g -std=c++20 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Iinclude tools/qrp_argcheck.cpp linearoperators.jl_amd/csrc/linalg.hip linearoperators.jl_amd/csrc/api_ctx.hip \
//       -o /tmp/qrp_argcheck && /tmp/qrp_argcheck
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
  const int64_t mf = 200, nf = 129, nb = 3, scratch_len = 2 * 64 * nf + 64 + 2 * nf + 2 * mf + 2 + 64 * 4096;
  std::vector<double> pool(8 * (mf + nf + 2 * 512 * 64) + mf * nf * 3 + 2 * nb * 4096 + scratch_len + 4096);
  double *p = pool.data();
  double *M = p; p += mf * nf;
  double *W = p; p += mf * nf;
  double *tfac = p; p += nb * 4096;
  double *dinv = p; p += nb * 4096;
  int32_t *jpvt = (int32_t *)p; p += nf;
  double *scratch = p; p += scratch_len;
  int32_t *info_dev = (int32_t *)p; p += 1;
  double *work = p; p += 8 * (mf + nf + 2 * 512 * 64);
  double *res = p; p += 8 * mf;
  double *v = p; p += 8 * mf;
  int32_t info = -1, rank = -1;
  const int32_t F64 = MXLO_F64, N = MXLO_OP_N, T = MXLO_OP_T;

  // ---- mxlo_geqp3
  expect("geqp3: null ctx", mxlo_geqp3(nullptr, F64, M, mf, 0, W, mf, mf, nf, tfac, dinv, jpvt, 1e-13, scratch, scratch_len, info_dev, &info, &rank), MXLO_EINVAL);
  expect("geqp3: complex dtype", mxlo_geqp3(&ctx, MXLO_C64, M, mf, 0, W, mf, mf, nf, tfac, dinv, jpvt, 1e-13, scratch, scratch_len, info_dev, &info, &rank), MXLO_EINVAL);
  expect("geqp3: nf > mf", mxlo_geqp3(&ctx, F64, M, mf, 0, W, mf, nf, mf, tfac, dinv, jpvt, 1e-13, scratch, scratch_len, info_dev, &info, &rank), MXLO_ESHAPE);
  expect("geqp3: nf == 0", mxlo_geqp3(&ctx, F64, M, mf, 0, W, mf, mf, 0, tfac, dinv, jpvt, 1e-13, scratch, scratch_len, info_dev, &info, &rank), MXLO_ESHAPE);
  expect("geqp3: ldw < mf", mxlo_geqp3(&ctx, F64, M, mf, 0, W, mf - 1, mf, nf, tfac, dinv, jpvt, 1e-13, scratch, scratch_len, info_dev, &info, &rank), MXLO_ESHAPE);
  expect("geqp3: mf too large", mxlo_geqp3(&ctx, F64, M, 1LL << 31, 0, W, 1LL << 31, 1LL << 31, nf, tfac, dinv, jpvt, 1e-13, scratch, scratch_len, info_dev, &info, &rank), MXLO_ESHAPE);
  expect("geqp3: rtol == 1", mxlo_geqp3(&ctx, F64, M, mf, 0, W, mf, mf, nf, tfac, dinv, jpvt, 1.0, scratch, scratch_len, info_dev, &info, &rank), MXLO_EINVAL);
  expect("geqp3: rtol < 0", mxlo_geqp3(&ctx, F64, M, mf, 0, W, mf, mf, nf, tfac, dinv, jpvt, -1e-3, scratch, scratch_len, info_dev, &info, &rank), MXLO_EINVAL);
  expect("geqp3: rtol NaN", mxlo_geqp3(&ctx, F64, M, mf, 0, W, mf, mf, nf, tfac, dinv, jpvt, __builtin_nan(""), scratch, scratch_len, info_dev, &info, &rank), MXLO_EINVAL);
  expect("geqp3: null M", mxlo_geqp3(&ctx, F64, nullptr, mf, 0, W, mf, mf, nf, tfac, dinv, jpvt, 1e-13, scratch, scratch_len, info_dev, &info, &rank), MXLO_EINVAL);
  expect("geqp3: null jpvt", mxlo_geqp3(&ctx, F64, M, mf, 0, W, mf, mf, nf, tfac, dinv, nullptr, 1e-13, scratch, scratch_len, info_dev, &info, &rank), MXLO_EINVAL);
  expect("geqp3: null rank", mxlo_geqp3(&ctx, F64, M, mf, 0, W, mf, mf, nf, tfac, dinv, jpvt, 1e-13, scratch, scratch_len, info_dev, &info, nullptr), MXLO_EINVAL);
  expect("geqp3: null info", mxlo_geqp3(&ctx, F64, M, mf, 0, W, mf, mf, nf, tfac, dinv, jpvt, 1e-13, scratch, scratch_len, info_dev, nullptr, &rank), MXLO_EINVAL);
  expect("geqp3: ldm < mf", mxlo_geqp3(&ctx, F64, M, mf - 1, 0, W, mf, mf, nf, tfac, dinv, jpvt, 1e-13, scratch, scratch_len, info_dev, &info, &rank), MXLO_ESHAPE);
  expect("geqp3: ldm < nf, transposed", mxlo_geqp3(&ctx, F64, M, nf - 1, 1, W, mf, mf, nf, tfac, dinv, jpvt, 1e-13, scratch, scratch_len, info_dev, &info, &rank), MXLO_ESHAPE);
  expect("geqp3: scratch too short", mxlo_geqp3(&ctx, F64, M, mf, 0, W, mf, mf, nf, tfac, dinv, jpvt, 1e-13, scratch, scratch_len - 1, info_dev, &info, &rank), MXLO_ESHAPE);
  expect("geqp3: W is M", mxlo_geqp3(&ctx, F64, M, mf, 0, M, mf, mf, nf, tfac, dinv, jpvt, 1e-13, scratch, scratch_len, info_dev, &info, &rank), MXLO_EINVAL);
  expect("geqp3: jpvt inside W", mxlo_geqp3(&ctx, F64, M, mf, 0, W, mf, mf, nf, tfac, dinv, (int32_t *)(W + 7), 1e-13, scratch, scratch_len, info_dev, &info, &rank), MXLO_EINVAL);
  expect("geqp3: jpvt inside the scratch", mxlo_geqp3(&ctx, F64, M, mf, 0, W, mf, mf, nf, tfac, dinv, (int32_t *)scratch + 5, 1e-13, scratch, scratch_len, info_dev, &info, &rank), MXLO_EINVAL);
  expect("geqp3: second info word inside jpvt", mxlo_geqp3(&ctx, F64, M, mf, 0, W, mf, mf, nf, tfac, dinv, jpvt, 1e-13, scratch, scratch_len, jpvt - 1, &info, &rank), MXLO_EINVAL);
  ctx.capturing = true;
  expect("geqp3: during a capture", mxlo_geqp3(&ctx, F64, M, mf, 0, W, mf, mf, nf, tfac, dinv, jpvt, 1e-13, scratch, scratch_len, info_dev, &info, &rank), MXLO_ESTATE);
  ctx.capturing = false;

  // ---- mxlo_qrp_mul
  expect("qrp_mul: null ctx", mxlo_qrp_mul(nullptr, F64, res, W, mf, mf, nf, tfac, dinv, jpvt, 65, work, v, N, 1.0, 0.0), MXLO_EINVAL);
  expect("qrp_mul: bad op_mode", mxlo_qrp_mul(&ctx, F64, res, W, mf, mf, nf, tfac, dinv, jpvt, 65, work, v, 77, 1.0, 0.0), MXLO_EINVAL);
  expect("qrp_mul: nf > mf", mxlo_qrp_mul(&ctx, F64, res, W, mf, nf, mf, tfac, dinv, jpvt, 65, work, v, N, 1.0, 0.0), MXLO_ESHAPE);
  expect("qrp_mul: rank 0", mxlo_qrp_mul(&ctx, F64, res, W, mf, mf, nf, tfac, dinv, jpvt, 0, work, v, N, 1.0, 0.0), MXLO_ESHAPE);
  expect("qrp_mul: rank > nf", mxlo_qrp_mul(&ctx, F64, res, W, mf, mf, nf, tfac, dinv, jpvt, nf + 1, work, v, N, 1.0, 0.0), MXLO_ESHAPE);
  expect("qrp_mul: null jpvt", mxlo_qrp_mul(&ctx, F64, res, W, mf, mf, nf, tfac, dinv, nullptr, 65, work, v, N, 1.0, 0.0), MXLO_EINVAL);
  expect("qrp_mul: null res", mxlo_qrp_mul(&ctx, F64, nullptr, W, mf, mf, nf, tfac, dinv, jpvt, 65, work, v, N, 1.0, 0.0), MXLO_EINVAL);
  expect("qrp_mul: res is v, rectangular", mxlo_qrp_mul(&ctx, F64, v, W, mf, mf, nf, tfac, dinv, jpvt, 65, work, v, N, 1.0, 0.0), MXLO_EINVAL);
  expect("qrp_mul: res overlaps v", mxlo_qrp_mul(&ctx, F64, v + 1, W, mf, mf, nf, tfac, dinv, jpvt, 65, work, v, T, 1.0, 0.0), MXLO_EINVAL);
  expect("qrp_mul: res inside jpvt", mxlo_qrp_mul(&ctx, F64, (double *)jpvt, W, mf, mf, nf, tfac, dinv, jpvt, 65, work, v, N, 1.0, 0.0), MXLO_EINVAL);
  expect("qrp_mul: v inside jpvt", mxlo_qrp_mul(&ctx, F64, res, W, mf, mf, nf, tfac, dinv, jpvt, 65, work, (double *)jpvt - mf + 1, N, 1.0, 0.0), MXLO_EINVAL);
  expect("qrp_mul: res inside the work vector", mxlo_qrp_mul(&ctx, F64, work + 3, W, mf, mf, nf, tfac, dinv, jpvt, 65, work, v, N, 1.0, 0.0), MXLO_EINVAL);

  // ---- mxlo_qrp_mul_block
  expect("qrp_mul_block: null ctx", mxlo_qrp_mul_block(nullptr, F64, res, nf, W, mf, mf, nf, tfac, dinv, jpvt, 65, work, v, mf, 8, N, 1.0, 0.0), MXLO_EINVAL);
  expect("qrp_mul_block: k == 0 launches nothing", mxlo_qrp_mul_block(&ctx, F64, nullptr, nf, W, mf, mf, nf, tfac, dinv, jpvt, 65, work, nullptr, mf, 0, N, 1.0, 0.0), MXLO_OK);
  expect("qrp_mul_block: k < 0", mxlo_qrp_mul_block(&ctx, F64, res, nf, W, mf, mf, nf, tfac, dinv, jpvt, 65, work, v, mf, -1, N, 1.0, 0.0), MXLO_ESHAPE);
  expect("qrp_mul_block: ldr < nf", mxlo_qrp_mul_block(&ctx, F64, res, nf - 1, W, mf, mf, nf, tfac, dinv, jpvt, 65, work, v, mf, 8, N, 1.0, 0.0), MXLO_ESHAPE);
  expect("qrp_mul_block: ldv < nf, transposed", mxlo_qrp_mul_block(&ctx, F64, res, mf, W, mf, mf, nf, tfac, dinv, jpvt, 65, work, v, nf - 1, 8, T, 1.0, 0.0), MXLO_ESHAPE);
  expect("qrp_mul_block: rank > nf", mxlo_qrp_mul_block(&ctx, F64, res, nf, W, mf, mf, nf, tfac, dinv, jpvt, nf + 1, work, v, mf, 8, N, 1.0, 0.0), MXLO_ESHAPE);
  expect("qrp_mul_block: null jpvt", mxlo_qrp_mul_block(&ctx, F64, res, nf, W, mf, mf, nf, tfac, dinv, nullptr, 65, work, v, mf, 8, N, 1.0, 0.0), MXLO_EINVAL);
  expect("qrp_mul_block: null V", mxlo_qrp_mul_block(&ctx, F64, res, nf, W, mf, mf, nf, tfac, dinv, jpvt, 65, work, nullptr, mf, 8, N, 1.0, 0.0), MXLO_EINVAL);
  expect("qrp_mul_block: res is V, rectangular", mxlo_qrp_mul_block(&ctx, F64, v, mf, W, mf, mf, nf, tfac, dinv, jpvt, 65, work, v, mf, 8, N, 1.0, 0.0), MXLO_EINVAL);
  expect("qrp_mul_block: last column of res inside jpvt", mxlo_qrp_mul_block(&ctx, F64, (double *)jpvt - 7 * nf, nf, W, mf, mf, nf, tfac, dinv, jpvt, 65, work, v, mf, 8, N, 1.0, 0.0), MXLO_EINVAL);
  expect("qrp_mul_block: V inside jpvt", mxlo_qrp_mul_block(&ctx, F64, res, mf, W, mf, mf, nf, tfac, dinv, jpvt, 65, work, (double *)jpvt, nf, 8, T, 1.0, 0.0), MXLO_EINVAL);
  expect("qrp_mul_block: res inside the work space", mxlo_qrp_mul_block(&ctx, F64, work + 8 * (mf + nf) + 5, nf, W, mf, mf, nf, tfac, dinv, jpvt, 65, work, v, mf, 8, N, 1.0, 0.0), MXLO_EINVAL);

  std::printf("%d unexpected\n", failures);
  return failures ? 1 : 0;
}
