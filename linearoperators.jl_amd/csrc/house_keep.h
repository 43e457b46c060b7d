// house_keep.h — the Householder dot launch at HBM sizes that keeps its last rounds on chip.
//
// mul!(res, opHouseholder(h), v) above the single-launch limit is a read-only dot pass (16 B/elt) and an update pass
// that re-reads h and v (24 B/elt). The dot pass runs ONE workgroup per CU with one wave per SIMD: each lane may use
// the whole 512-register budget and the CU's 160 KiB of LDS are idle. Here every workgroup keeps the h and v vectors
// of its last KL + KR grid-stride rounds (KL in LDS, KR in registers), the workgroups exchange their partial sums as
// the single-launch form does (GridExchange, grid_exchange.h, on the same slots), and each one updates what it
// kept. Those rounds are one contiguous tail of the vector (house_keep_plan.h), so the update launch simply gets a
// shorter n: 40 - 16 kept/n bytes per element, and no finalize launch.
//
// Bits: chunk -> workgroup assignment, per-lane FMA order, scalar head/tail, wave_sum and the four-wave sum are those
// of panel_dots_kernel<T, VEC, 1, 4, true, true>; the partials are summed in finalize_kernel's order; the update is
// HouseholderOp. Results are bit-identical to the three-launch path.
#pragma once
#include "common.h"
#include "house_keep_plan.h"
#include "stream_kernels.h"

namespace mxlo {

// Rounds kept per workgroup. One round is 256 lanes x 4 vectors x 16 B = 16 KiB per stream: 32 VGPRs per lane for h
// and v together, or 32 KiB of LDS. 14 + 4 is the largest candidate that compiles without scratch (256 VGPRs + 216-240
// AGPRs, 128 KiB of LDS) and the fastest of the six measured at every swept size (profiles/house_keep.md: house_fused 1
// against 0 at n = 1e8 f64, KR/KL 8/0 2.0 %, 12/0 2.9 %, 14/0 2.7 %, 8/4 2.7 %, 12/4 3.3 %, 14/4 3.8 %).
constexpr int kHouseKeepKR = 14;
constexpr int kHouseKeepKL = 4;
constexpr int kHouseKeepUnroll = 4;   // = launch_dots' UNROLL for one column
static_assert(kHouseKeepUnroll == kStreamUnroll, "the dot launch and the update launch count the same chunks");

// The slice of h that stays in the Infinity Cache between applies (house_keep_plan.h: house_resident_q / _chunk): its
// target is this many sixteenths of Tune::nt_min_bytes, the key that stands for the cache's size. 0 switches it off.
// profiles/house_resident.md, house_fused 1 against 0 in one process at n = 1e8 f64 (the parent: 4.3-4.5 %): 0 4.2-4.9 %,
// 4 4.9-5.1 %, 8 6.2-6.5 %, 10 7.4 %, 12 8.5-8.8 %, 14 8.7-8.8 % (12 and 14 are the same 4 sixteenths = 200 MB there);
// 14 is also the fastest at n = 5e7 f64 and 1e8 f32, where 12 lands on 8 sixteenths — every other diagonal — and gains nothing.
constexpr int kHouseResidentNum = 14;
static_assert(kHouseResidentNum >= 0 && kHouseResidentNum <= 16);
// The two sides of a per-chunk policy choice load the same addresses and differ only in the nontemporal hint, which is
// metadata: when the compiler merges the "identical" loads of the two sides it drops the hint and EVERY load of h takes
// the default policy (seen in the ISA). A side-effecting marker that differs between the sides, in front of and behind
// the loads, keeps them two straight lines; it emits a comment, no instruction and no wait.
#define MXLO_POLICY_SIDE(tag) asm volatile("; h loads: " tag ::: "memory")
struct HouseResident {
  int q = 0;      // sixteenths of h's chunks loaded with the default policy; 0: every load nontemporal, as before
  int grid = 0;   // workgroups of the dot launch: chunk c is round c / grid, workgroup c % grid
};

template <typename T, typename CA, typename CB, bool BETA0, int KR, int KL>
__global__ void __launch_bounds__(kBlock)
householder_dots_keep_kernel(T *__restrict__ res, const T *__restrict__ h, const T *__restrict__ v, int64_t head,
                             int64_t n, CA alpha, CB beta, HouseKeepPlan pl, unsigned long long *__restrict__ slots,
                             unsigned long long ticks, unsigned *__restrict__ fault, int drop,
                             double *__restrict__ dot_out, int rq) {
  constexpr int VEC = Vec16<T>::N, U = kHouseKeepUnroll;
  using V = typename Vec16<T>::type;
  constexpr int64_t CHUNK = (int64_t)kBlock * U;
  extern __shared__ __attribute__((aligned(16))) unsigned char keep_lds[];   // [2][KL][U][kBlock] vectors: h, then v
  V *lh = reinterpret_cast<V *>(keep_lds), *lx = lh + (int64_t)KL * CHUNK;
  const int tid = threadIdx.x, G = (int)gridDim.x, b = (int)blockIdx.x;
  GridExchange X;
  X.begin<kBlock>(slots, kFusedSlots);

  const V *hv = reinterpret_cast<const V *>(h + head), *xv = reinterpret_cast<const V *>(v + head);
  V *rv = reinterpret_cast<V *>(res + head);
  double acc = 0.0;
  auto load4 = [&](int64_t round, V (&a)[U], V (&x)[U]) {
    const int64_t base = (round * G + b) * CHUNK + tid;
    // a resident chunk of h takes the default policy: one wave-uniform choice per chunk, each side a straight line of loads
    if (house_resident_diag((int)((round + b) & 15), rq)) {
      MXLO_POLICY_SIDE("resident");
#pragma unroll
      for (int u = 0; u < U; ++u) {
        x[u] = __builtin_nontemporal_load(xv + base + (int64_t)u * kBlock);
        a[u] = hv[base + (int64_t)u * kBlock];
      }
      MXLO_POLICY_SIDE("resident, issued");
    } else {
      MXLO_POLICY_SIDE("streamed");
#pragma unroll
      for (int u = 0; u < U; ++u) {
        x[u] = __builtin_nontemporal_load(xv + base + (int64_t)u * kBlock);
        a[u] = __builtin_nontemporal_load(hv + base + (int64_t)u * kBlock);
      }
      MXLO_POLICY_SIDE("streamed, issued");
    }
  };
  auto fma4 = [&](const V (&a)[U], const V (&x)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc = fma((double)a[u][k], (double)x[u][k], acc);
  };
  for (int64_t r = 0; r < pl.first; ++r) {   // streamed rounds
    V a[U], x[U];
    load4(r, a, x);
    fma4(a, x);
  }
  if constexpr (KL > 0) {
#pragma unroll 1
    for (int q = 0; q < pl.kl; ++q) {        // rounds kept in LDS: every lane parks (and later reads) its own vectors
      V a[U], x[U];
      load4(pl.first + q, a, x);
      fma4(a, x);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        lh[(q * U + u) * kBlock + tid] = a[u];
        lx[(q * U + u) * kBlock + tid] = x[u];
      }
    }
  }
  V kh[KR][U], kx[KR][U];                    // rounds kept in registers: every load issued before the first FMA
  const int64_t reg0 = pl.first + pl.kl;
#pragma unroll
  for (int q = 0; q < KR; ++q)
    if (q < pl.kr) load4(reg0 + q, kh[q], kx[q]);
#pragma unroll
  for (int q = 0; q < KR; ++q)
    if (q < pl.kr) fma4(kh[q], kx[q]);
  // behind the last complete round: at most one (possibly partial) chunk per workgroup, then the scalar head / tail
  const int64_t rem = pl.rem_vec + (int64_t)b * CHUNK + tid;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = rem + (int64_t)u * kBlock;
    if (i < pl.nvec) {
      const V x = __builtin_nontemporal_load(xv + i), a = __builtin_nontemporal_load(hv + i);
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc = fma((double)a[k], (double)x[k], acc);
    }
  }
  const int64_t tail0 = head + pl.nvec * VEC, cnt = head + (n - tail0);
  if (b == G - 1 && tid < cnt) {
    const int64_t i = tid < head ? tid : tail0 + (tid - head);
    acc = fma((double)h[i], (double)v[i], acc);
  }

  __shared__ double lds[kBlock / kWave];
  const double s = block_sum4(acc, lds);
  if (tid == 0) X.publish(b, s, b == drop);
  // every workgroup waits for all G partials and adds them up in finalize_kernel's order (0 + slot t + slot t + 256 ..)
  double p = 0.0;
  for (int i = tid; i < G; i += kBlock) p += X.wait(i, ticks, fault, kFaultHouseholder);
  __syncthreads();                                                     // lds reuse
  const double dot = block_sum4(p, lds);
  if (b == 0 && tid == 0) *dot_out = dot;                              // for the update launch over the prefix
  X.finish();

  HouseholderOp<T, CA, CB, BETA0> op{alpha, beta, nullptr, T(0)};
  op.c = (T)2 * (T)dot;                                                // = HouseholderOp::init()
  auto update4 = [&](int64_t round, const V (&a)[U], const V (&x)[U]) {
    const int64_t base = (round * G + b) * CHUNK + tid;
    V r[U];
    if constexpr (!BETA0) {
#pragma unroll
      for (int u = 0; u < U; ++u) r[u] = __builtin_nontemporal_load(rv + base + (int64_t)u * kBlock);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      V o;
#pragma unroll
      for (int k = 0; k < VEC; ++k) o[k] = op(a[u][k], x[u][k], BETA0 ? T(0) : r[u][k]);
      __builtin_nontemporal_store(o, rv + base + (int64_t)u * kBlock);
    }
  };
#pragma unroll
  for (int q = 0; q < KR; ++q)
    if (q < pl.kr) update4(reg0 + q, kh[q], kx[q]);
  if constexpr (KL > 0) {
#pragma unroll 1
    for (int q = 0; q < pl.kl; ++q) {
      V a[U], x[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        a[u] = lh[(q * U + u) * kBlock + tid];
        x[u] = lx[(q * U + u) * kBlock + tid];
      }
      update4(pl.first + q, a, x);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {              // the remainder is read again: under 4 MiB per stream
    const int64_t i = rem + (int64_t)u * kBlock;
    if (i < pl.nvec) {
      const V x = xv[i], a = hv[i];
      V r, o;
      if constexpr (!BETA0) r = rv[i];
#pragma unroll
      for (int k = 0; k < VEC; ++k) o[k] = op(a[k], x[k], BETA0 ? T(0) : r[k]);
      __builtin_nontemporal_store(o, rv + i);
    }
  }
  if (b == G - 1 && tid >= head && tid < cnt) {                        // scalar tail; the head belongs to the prefix
    const int64_t i = tail0 + (tid - head);
    res[i] = op(h[i], v[i], BETA0 ? T(0) : res[i]);
  }
}

// The dot of a Householder apply into `dot`. When the kept form engages, it has also updated res[*n_left, n) and
// *n_left is the prefix the update launch still has to do; otherwise panel_dots runs as before and *n_left stays n.
// *rs: the resident slice of h the kept form loaded with the default policy (q = 0: none), for the update launch.
template <typename T>
static int32_t householder_dots_t(mxlo_ctx *ctx, T *res, const T *h, const T *v, int64_t *n_left, double alpha,
                                  double beta, int32_t flags, double *dot, HouseResident *rs) {
  constexpr int VEC = Vec16<T>::N, KR = kHouseKeepKR, KL = kHouseKeepKL;
  constexpr int64_t CHUNK = (int64_t)kBlock * kHouseKeepUnroll;
  constexpr size_t kLds = (size_t)2 * KL * CHUNK * 16;
  const int64_t n = *n_left;
  const T *cols[1] = {h};
  const int64_t head = common_head<T>({res, h, v});
  // a form whose workgroups wait for each other: the conditions of the single-launch form (house_fused, no all-reduce
  // hook, the fault word), and only where today's dot launch already is num_cu persistent workgroups on nontemporal loads
  bool keep = ctx->tune.house_fused && !ctx->allreduce && ctx->fault_dev && n > ctx->tune.house_inline_n && head >= 0 &&
              n >= 4 * VEC && (int64_t)sizeof(T) * n * 2 >= ctx->tune.nt_min_bytes;
  HouseKeepPlan pl;
  int grid = 0;
  if (keep) {
    const int per_cu = ctx->tune.red_blocks_per_cu > 1 ? 1 : ctx->tune.red_blocks_per_cu;   // = launch_dots, nontemporal, one column
    grid = grid_for(ctx, (n - head) / VEC, CHUNK, per_cu);
    pl = house_keep_plan(n, head, VEC, grid, CHUNK, KR, KL);
    keep = grid == ctx->num_cu && grid <= kFusedSlots && pl.ok;
  }
  if (!keep) return panel_dots<T>(ctx, cols, 1, v, n, dot);   // (+ all-reduce hook)
  const int rq = house_resident_q((int64_t)sizeof(T) * n, ctx->tune.nt_min_bytes / 16 * kHouseResidentNum);
  bool launched = false;
  MXLO_TRY((dispatch_ab<T>(beta, flags, [&]<typename CA, typename CB, bool B0>() -> int32_t {
    constexpr auto kernel = householder_dots_keep_kernel<T, CA, CB, B0, KR, KL>;
    static std::atomic<int> lds_cap[64];              // dynamic-LDS cap raised once per (instantiation, device): 1 set, 2 refused
    const int d = ctx->device & 63;
    int st = kLds > 48 * 1024 ? lds_cap[d].load(std::memory_order_relaxed) : 1;
    if (st == 0) {
      st = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds) == hipSuccess ? 1 : 2;
      if (st == 2) (void)hipGetLastError();
      lds_cap[d].store(st, std::memory_order_relaxed);
    }
    if (st != 1 || !coresident<kernel>(ctx, grid, kLds)) return MXLO_OK;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), kLds, ctx->stream, res, h, v, head, n, (CA)alpha, (CB)beta, pl,
                       ctx->xslots, fused_timeout_ticks(ctx), ctx->fault_dev, ctx->tune.fused_debug_drop, dot, rq);
    MXLO_LAUNCH_CHECK();
    launched = true;
    return MXLO_OK;
  })));
  if (!launched) return panel_dots<T>(ctx, cols, 1, v, n, dot);
  *n_left = pl.prefix;
  *rs = HouseResident{rq, grid};
  return MXLO_OK;
}

// The update launch over the prefix the kept form left, when that form loaded a resident slice of h (rs.q > 0): it is
// map_kernel<T, VEC, kStreamUnroll, 2, !BETA0, REVERSE, NT, HouseholderOp> — same chunks, same order, same arithmetic
// — with the h loads of the resident chunks on the default policy. The prefix is the scalar head and whole chunks.
template <typename T, typename CA, typename CB, bool BETA0, bool REVERSE, bool NT>
__global__ void __launch_bounds__(kBlock)
householder_update_resident_kernel(T *__restrict__ res, const T *__restrict__ h, const T *__restrict__ v, int64_t head,
                                   int64_t nchunks, int64_t dots_grid, int rq, HouseholderOp<T, CA, CB, BETA0> op) {
  constexpr int VEC = Vec16<T>::N, U = kStreamUnroll;
  using V = typename Vec16<T>::type;
  constexpr int64_t CHUNK = (int64_t)kBlock * U;
  op.init();
  const int tid = threadIdx.x;
  V *rv = reinterpret_cast<V *>(res + head);
  const V *hv = reinterpret_cast<const V *>(h + head), *xv = reinterpret_cast<const V *>(v + head);
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int64_t c = REVERSE ? (nchunks - 1 - ch) : ch;
    const int64_t base = c * CHUNK + tid;
    V a[U], x[U], r[U];
    if (house_resident_chunk(c, dots_grid, rq)) {   // wave-uniform; each side a straight line of loads
      MXLO_POLICY_SIDE("resident");
#pragma unroll
      for (int u = 0; u < U; ++u) {
        a[u] = hv[base + (int64_t)u * kBlock];
        x[u] = ldg<NT>(xv + base + (int64_t)u * kBlock);
        if constexpr (!BETA0) r[u] = ldg<NT>(rv + base + (int64_t)u * kBlock);
      }
      MXLO_POLICY_SIDE("resident, issued");
    } else {
      MXLO_POLICY_SIDE("streamed");
#pragma unroll
      for (int u = 0; u < U; ++u) {
        a[u] = ldg<NT>(hv + base + (int64_t)u * kBlock);
        x[u] = ldg<NT>(xv + base + (int64_t)u * kBlock);
        if constexpr (!BETA0) r[u] = ldg<NT>(rv + base + (int64_t)u * kBlock);
      }
      MXLO_POLICY_SIDE("streamed, issued");
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      V o;
#pragma unroll
      for (int k = 0; k < VEC; ++k) o[k] = op(a[u][k], x[u][k], BETA0 ? T(0) : r[u][k]);
      stg<NT>(rv + base + (int64_t)u * kBlock, o);
    }
  }
  if (blockIdx.x == gridDim.x - 1 && tid < head) res[tid] = op(h[tid], v[tid], BETA0 ? T(0) : res[tid]);   // scalar head
}

template <typename T>
static int32_t householder_apply_resident_t(mxlo_ctx *ctx, T *res, const T *h, const T *v, int64_t n, double alpha,
                                            double beta, int32_t flags, const double *dot, HouseResident rs) {
  constexpr int VEC = Vec16<T>::N;
  constexpr int64_t CHUNK = (int64_t)kBlock * kStreamUnroll;
  const int64_t head = common_head<T>({res, h, v}), nchunks = (n - head) / VEC / CHUNK;
  MXLO_REQUIRE(head >= 0 && rs.grid > 0 && head + nchunks * CHUNK * VEC == n, MXLO_ESTATE,
               "householder: the prefix of the kept form is not the scalar head and whole chunks");
  const bool rev = ctx->tune.house_reverse != 0;
  int64_t g = nchunks;                                   // = launch_map's grid and nontemporal rule
  if (ctx->tune.blocks_per_cu > 0 && g > (int64_t)ctx->num_cu * ctx->tune.blocks_per_cu) g = (int64_t)ctx->num_cu * ctx->tune.blocks_per_cu;
  const int grid = (int)(g > 0x7fffffffLL ? 0x7fffffffLL : (g < 1 ? 1 : g));
  return dispatch_ab<T>(beta, flags, [&]<typename CA, typename CB, bool B0>() -> int32_t {
    HouseholderOp<T, CA, CB, B0> op{(CA)alpha, (CB)beta, dot, T(0)};
    const bool nt = (int64_t)sizeof(T) * n * (B0 ? 3 : 4) >= ctx->tune.nt_min_bytes;
    auto go = [&]<bool REV, bool NT>() {
      hipLaunchKernelGGL((householder_update_resident_kernel<T, CA, CB, B0, REV, NT>), dim3(grid), dim3(kBlock), 0,
                         ctx->stream, res, h, v, head, nchunks, (int64_t)rs.grid, rs.q, op);
    };
    if (rev) nt ? go.template operator()<true, true>() : go.template operator()<true, false>();
    else nt ? go.template operator()<false, true>() : go.template operator()<false, false>();
    MXLO_LAUNCH_CHECK();
    return MXLO_OK;
  });
}

}  // namespace mxlo
