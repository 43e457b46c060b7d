// krylov.hip — the Gram–Schmidt step and the restart combination of a Lanczos / Arnoldi process on device vectors
// (estimate_opnorm: what ARPACK's reverse-communication loop does between two operator applies).
//
// mxlo_krylov_orth: w <- (I - V V')^2 w, normalised — classical Gram–Schmidt with one re-orthogonalisation round (CGS2)
// against the n x k orthonormal basis V. One round is two passes:
//   dots    h = V'w        every column and w read once per group of <= kKryNC columns, f64 accumulators per lane,
//                          wave_sum -> LDS -> one partial per (column, workgroup), fixed-order finalize (reductions.hip);
//   update  w -= V h       the same groups; s = sum_c V[i,c] h[c] is accumulated in f64 and subtracted from w ONCE (one
//                          rounding at the magnitude of w, as a BLAS gemv + axpy has). The pass that touches w first also
//                          sums w_old^2, the one that touches it last sums w_new^2 (of the STORED values): the DGKS test
//                          and beta need no pass of their own.
// A one-workgroup finish kernel turns the partial sums into coef[] and the DGKS flag; the kernels of the second round read
// that flag from device memory and return at once when it is set — the host never sees it. A last pass divides by beta.
// Everything is stream-ordered on the ctx stream: no allocation, no copy, no synchronisation, no float atomics; results
// are bit-reproducible (fixed chunk -> lane -> tree decomposition, independent of dispatch order).
//
// mxlo_krylov_combine: out = V y, normalised (the explicit restart vector). One kernel walks ALL k columns for the elements
// a lane owns before it stores them, so `out` may be a column of V itself.
#include "common.h"

namespace mxlo {
namespace {

constexpr int kKryNC = 10;            // columns per dots / update launch (register-sized group)
constexpr int kKryNCScalar = 4;       // ... on the element-wise path (columns of different 16-byte phases)
constexpr int kKryMaxK = 128;         // basis columns one call accepts (= kMaxRedCols)
constexpr int kKryScalars = 4096;     // ctx->scalars + this: h[kKryMaxK], w_old^2, w_new^2, skip flag (transient, stream-ordered)
constexpr int kKryBefore = kKryMaxK, kKryAfter = kKryMaxK + 1, kKrySkip = kKryMaxK + 2;

template <typename T, int VEC>
using KVec = typename std::conditional<VEC == 1, T, typename Vec16<T>::type>::type;

template <typename T, int VEC, bool NT>
__device__ __forceinline__ KVec<T, VEC> kld(const T *p) {
  using V = KVec<T, VEC>;
  if constexpr (VEC == 1) return *p;
  else return NT ? __builtin_nontemporal_load(reinterpret_cast<const V *>(p)) : *reinterpret_cast<const V *>(p);
}
template <typename T, int VEC>
__device__ __forceinline__ T kelt(const KVec<T, VEC> &v, int e) {
  if constexpr (VEC == 1) return v;
  else return v[e];
}
// w: vector access when it shares V's 16-byte phase (WVEC), element accesses otherwise; never nontemporal (the next pass reads it again)
template <typename T, int VEC, bool WVEC>
__device__ __forceinline__ void kld_w(const T *p, T (&xe)[VEC]) {
  if constexpr (VEC > 1 && WVEC) {
    const KVec<T, VEC> xv = *reinterpret_cast<const KVec<T, VEC> *>(p);
#pragma unroll
    for (int e = 0; e < VEC; ++e) xe[e] = xv[e];
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) xe[e] = p[e];
  }
}
template <typename T, int VEC, bool WVEC>
__device__ __forceinline__ void kst_w(T *p, const T (&xe)[VEC]) {
  if constexpr (VEC > 1 && WVEC) {
    KVec<T, VEC> xv;
#pragma unroll
    for (int e = 0; e < VEC; ++e) xv[e] = xe[e];
    *reinterpret_cast<KVec<T, VEC> *>(p) = xv;
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) p[e] = xe[e];
  }
}

// workgroup sum of NP per-lane doubles -> partials[p][blockIdx.x] (the layout finalize reads)
template <int NP>
__device__ __forceinline__ void block_partials(const double (&acc)[NP], double *__restrict__ partials, unsigned keep = ~0u) {
  __shared__ double lds[kBlock / kWave][NP];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const double s = wave_sum(acc[p]);
    if (lane == 0) lds[wave][p] = s;
  }
  __syncthreads();
  if (tid < NP && ((keep >> tid) & 1u))
    partials[(int64_t)tid * kMaxRedBlocks + blockIdx.x] = (lds[0][tid] + lds[1][tid]) + (lds[2][tid] + lds[3][tid]);
}

// ---- dots: partials[c][wg] = sum over the workgroup's chunks of V[:, c] .* w, c < NC ------------------------------------
// Elements [head, head + nvec * VEC) are walked as 16-byte vectors of V (all columns share V's phase: ldv is a multiple
// of the vector width), the < 2 VEC elements in front of and behind them by the last workgroup, one per lane.
template <typename T, int VEC, int NC, int UNROLL, bool WVEC, bool NT>
__global__ void __launch_bounds__(kBlock)
korth_dots_kernel(const T *__restrict__ V, int64_t ldv, const T *__restrict__ w, int64_t head, int64_t nvec, int64_t n,
                  double *__restrict__ partials, const double *__restrict__ skip) {
  if (skip && *skip != 0.0) return;   // DGKS: the second round is not needed (decided by korth_finish_kernel, on the device)
  using VT = KVec<T, VEC>;
  const int tid = threadIdx.x;
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  auto accumulate = [&](const VT (&cv)[NC], const T (&xe)[VEC]) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[c] = fma((double)kelt<T, VEC>(cv[c], e), (double)xe[e], acc[c]);
  };
  constexpr int64_t CHUNK = (int64_t)kBlock * UNROLL;
  const int64_t nchunks = (nvec + CHUNK - 1) / CHUNK;
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int64_t base = ch * CHUNK + tid;
    if (base + (int64_t)(UNROLL - 1) * kBlock < nvec) {   // whole chunk in range: every load issued before the first FMA
      T xe[UNROLL][VEC];
      VT cv[UNROLL][NC];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t off = head + (base + (int64_t)u * kBlock) * VEC;
        kld_w<T, VEC, WVEC>(w + off, xe[u]);
#pragma unroll
        for (int c = 0; c < NC; ++c) cv[u][c] = kld<T, VEC, NT>(V + (int64_t)c * ldv + off);
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) accumulate(cv[u], xe[u]);
    } else {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t i = base + (int64_t)u * kBlock;
        if (i < nvec) {
          const int64_t off = head + i * VEC;
          T xe[VEC];
          VT cv[NC];
          kld_w<T, VEC, WVEC>(w + off, xe);
#pragma unroll
          for (int c = 0; c < NC; ++c) cv[c] = kld<T, VEC, NT>(V + (int64_t)c * ldv + off);
          accumulate(cv, xe);
        }
      }
    }
  }
  if constexpr (VEC > 1) {
    if (blockIdx.x == gridDim.x - 1) {
      const int64_t tail0 = head + nvec * VEC;
      const int64_t cnt = head + (n - tail0);
      if (tid < cnt) {
        const int64_t i = tid < head ? tid : tail0 + (tid - head);
        const double xe = (double)w[i];
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = fma((double)V[(int64_t)c * ldv + i], xe, acc[c]);
      }
    }
  }
  block_partials<NC>(acc, partials);
}

// one workgroup per column: out[c] = sum of its partials, lane t adding t, t + 256, ... then the fixed tree (finalize_kernel's order)
__device__ __forceinline__ double sum_partials(const double *__restrict__ p, int nblocks, double *lds) {
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < nblocks; i += kBlock) s += p[i];
  s = wave_sum(s);
  __syncthreads();   // lds reuse
  if ((tid & 63) == 0) lds[tid >> 6] = s;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}
__global__ void __launch_bounds__(kBlock)
kry_finalize_kernel(const double *__restrict__ partials, int nblocks, double *__restrict__ out, const double *__restrict__ skip,
                    int take_sqrt) {
  if (skip && *skip != 0.0) return;
  __shared__ double lds[kBlock / kWave];
  const double v = sum_partials(partials + (int64_t)blockIdx.x * kMaxRedBlocks, nblocks, lds);
  if (threadIdx.x == 0) out[blockIdx.x] = take_sqrt ? sqrt(v) : v;
}

// ---- update: w -= V[:, 0..NC) h; partial row 0 = sum w_old^2 (first group), row 1 = sum w_new^2 (last group) --------------
template <typename T, int VEC, int NC, int UNROLL, bool WVEC, bool NT>
__global__ void __launch_bounds__(kBlock)
korth_update_kernel(const T *__restrict__ V, int64_t ldv, T *__restrict__ w, int64_t head, int64_t nvec, int64_t n,
                    const double *__restrict__ h, double *__restrict__ partials, int first, int last,
                    const double *__restrict__ skip) {
  if (skip && *skip != 0.0) return;
  using VT = KVec<T, VEC>;
  const int tid = threadIdx.x;
  double hc[NC], acc[2] = {0.0, 0.0};
#pragma unroll
  for (int c = 0; c < NC; ++c) hc[c] = h[c];
  auto update = [&](const VT (&cv)[NC], T (&xe)[VEC]) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double wo = (double)xe[e];
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < NC; ++c) s = fma((double)kelt<T, VEC>(cv[c], e), hc[c], s);
      xe[e] = (T)(wo - s);
      acc[0] = fma(wo, wo, acc[0]);
      acc[1] = fma((double)xe[e], (double)xe[e], acc[1]);
    }
  };
  constexpr int64_t CHUNK = (int64_t)kBlock * UNROLL;
  const int64_t nchunks = (nvec + CHUNK - 1) / CHUNK;
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int64_t base = ch * CHUNK + tid;
    if (base + (int64_t)(UNROLL - 1) * kBlock < nvec) {
      T xe[UNROLL][VEC];
      VT cv[UNROLL][NC];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t off = head + (base + (int64_t)u * kBlock) * VEC;
        kld_w<T, VEC, WVEC>(w + off, xe[u]);
#pragma unroll
        for (int c = 0; c < NC; ++c) cv[u][c] = kld<T, VEC, NT>(V + (int64_t)c * ldv + off);
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        update(cv[u], xe[u]);
        kst_w<T, VEC, WVEC>(w + head + (base + (int64_t)u * kBlock) * VEC, xe[u]);
      }
    } else {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t i = base + (int64_t)u * kBlock;
        if (i < nvec) {
          const int64_t off = head + i * VEC;
          T xe[VEC];
          VT cv[NC];
          kld_w<T, VEC, WVEC>(w + off, xe);
#pragma unroll
          for (int c = 0; c < NC; ++c) cv[c] = kld<T, VEC, NT>(V + (int64_t)c * ldv + off);
          update(cv, xe);
          kst_w<T, VEC, WVEC>(w + off, xe);
        }
      }
    }
  }
  if constexpr (VEC > 1) {
    if (blockIdx.x == gridDim.x - 1) {
      const int64_t tail0 = head + nvec * VEC;
      const int64_t cnt = head + (n - tail0);
      if (tid < cnt) {
        const int64_t i = tid < head ? tid : tail0 + (tid - head);
        const double wo = (double)w[i];
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) s = fma((double)V[(int64_t)c * ldv + i], hc[c], s);
        const T wn = (T)(wo - s);
        w[i] = wn;
        acc[0] = fma(wo, wo, acc[0]);
        acc[1] = fma((double)wn, (double)wn, acc[1]);
      }
    }
  }
  block_partials<2>(acc, partials, (first ? 1u : 0u) | (last ? 2u : 0u));
}

// ---- finish of a round (ONE workgroup): coefficients, beta and the DGKS decision ------------------------------------------
//   round 1: coef[c] = h[c], coef[k] = |w_new|, ws[skip] = (|w_new| >= |w_old| / sqrt 2) — compared as 2 |w_new|^2 >= |w_old|^2;
//   round 2: coef[c] += h[c], coef[k] = |w_new|  (nothing at all when the round was skipped).
__global__ void __launch_bounds__(kBlock)
korth_finish_kernel(const double *__restrict__ partials, int nb_before, int nb_after, double *__restrict__ ws, int k, double *__restrict__ coef,
                    int round, const double *__restrict__ skip) {
  if (skip && *skip != 0.0) return;
  __shared__ double lds[kBlock / kWave];
  const int tid = threadIdx.x;
  const double after2 = sum_partials(partials + kMaxRedBlocks, nb_after, lds);
  if (round == 1) {
    const double before2 = sum_partials(partials, nb_before, lds);
    if (tid == 0) {
      ws[kKryBefore] = before2;
      ws[kKrySkip] = (2.0 * after2 >= before2) ? 1.0 : 0.0;   // NaN: not skipped, the second round carries it on
    }
    if (tid < k) coef[tid] = ws[tid];
  } else if (tid < k) {
    coef[tid] += ws[tid];
  }
  if (tid == 0) {
    ws[kKryAfter] = after2;
    coef[k] = sqrt(after2);
  }
}

// ---- x ./= *beta unless beta is 0 or not finite (breakdown: the vector stays as it is, the host decides) -----------------
template <typename T, int VEC>
__global__ void __launch_bounds__(kBlock)
kry_normalise_kernel(T *__restrict__ x, int64_t head, int64_t nvec, int64_t n, const double *__restrict__ beta) {
  using VT = KVec<T, VEC>;
  const double b = *beta;
  if (!(b > 0.0) || !(b <= 1.7976931348623157e308)) return;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * kBlock) {
    VT *p = reinterpret_cast<VT *>(x + head) + i;
    if constexpr (VEC == 1) {
      *p = (T)((double)*p / b);   // a true division, rounded once to T
    } else {
      VT v = *p;
#pragma unroll
      for (int e = 0; e < VEC; ++e) v[e] = (T)((double)v[e] / b);
      *p = v;
    }
  }
  if constexpr (VEC > 1) {
    if (blockIdx.x == gridDim.x - 1) {
      const int64_t tail0 = head + nvec * VEC;
      const int64_t cnt = head + (n - tail0);
      if (threadIdx.x < cnt) {
        const int64_t i = (int64_t)threadIdx.x < head ? threadIdx.x : tail0 + (threadIdx.x - head);
        x[i] = (T)((double)x[i] / b);
      }
    }
  }
}

// ---- combine: out = V[:, 0..k) y, partial row 0 = sum out^2 ----------------------------------------------------------------
// No __restrict__: out may BE a column of V. A lane reads all k columns at its elements before it stores them, and no
// other lane ever touches those elements, so the alias is harmless by ordering.
template <typename T, int VEC, bool OVEC, bool NT>
__global__ void __launch_bounds__(kBlock)
kry_combine_kernel(const T *V, int64_t ldv, int k, const double *__restrict__ y, T *out, int64_t head, int64_t nvec, int64_t n,
                   double *__restrict__ partials) {
  using VT = KVec<T, VEC>;
  constexpr int NCB = 8;   // columns in flight per lane
  const int tid = threadIdx.x;
  double acc[1] = {0.0};
  for (int64_t i = (int64_t)blockIdx.x * kBlock + tid; i < nvec; i += (int64_t)gridDim.x * kBlock) {
    const int64_t off = head + i * VEC;
    double s[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) s[e] = 0.0;
    int c0 = 0;
    for (; c0 + NCB <= k; c0 += NCB) {
      VT cv[NCB];
#pragma unroll
      for (int c = 0; c < NCB; ++c) cv[c] = kld<T, VEC, NT>(V + (int64_t)(c0 + c) * ldv + off);
#pragma unroll
      for (int c = 0; c < NCB; ++c) {
        const double yc = y[c0 + c];
#pragma unroll
        for (int e = 0; e < VEC; ++e) s[e] = fma((double)kelt<T, VEC>(cv[c], e), yc, s[e]);
      }
    }
    for (; c0 < k; ++c0) {
      const VT cv = kld<T, VEC, NT>(V + (int64_t)c0 * ldv + off);
      const double yc = y[c0];
#pragma unroll
      for (int e = 0; e < VEC; ++e) s[e] = fma((double)kelt<T, VEC>(cv, e), yc, s[e]);
    }
    T xe[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      xe[e] = (T)s[e];
      acc[0] = fma((double)xe[e], (double)xe[e], acc[0]);
    }
    kst_w<T, VEC, OVEC>(out + off, xe);
  }
  if constexpr (VEC > 1) {
    if (blockIdx.x == gridDim.x - 1) {
      const int64_t tail0 = head + nvec * VEC;
      const int64_t cnt = head + (n - tail0);
      if (tid < cnt) {
        const int64_t i = tid < head ? tid : tail0 + (tid - head);
        double s = 0.0;
        for (int c = 0; c < k; ++c) s = fma((double)V[(int64_t)c * ldv + i], y[c], s);
        const T o = (T)s;
        out[i] = o;
        acc[0] = fma((double)o, (double)o, acc[0]);
      }
    }
  }
  block_partials<1>(acc, partials);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
template <typename F>
inline void with_nc(int nc, F &&f) {
  switch (nc) {
    case 1: f.template operator()<1>(); break;
    case 2: f.template operator()<2>(); break;
    case 3: f.template operator()<3>(); break;
    case 4: f.template operator()<4>(); break;
    case 5: f.template operator()<5>(); break;
    case 6: f.template operator()<6>(); break;
    case 7: f.template operator()<7>(); break;
    case 8: f.template operator()<8>(); break;
    case 9: f.template operator()<9>(); break;
    default: f.template operator()<10>(); break;
  }
}

// how a basis of columns V + c * ldv and a vector of length n are walked: 16-byte vectors from `head` on when every column
// shares one phase, element by element otherwise
template <typename T>
struct Walk {
  bool vec;
  int64_t head, nvec;
  Walk(const T *V, int64_t ldv, int k, int64_t n) {
    constexpr int VEC = Vec16<T>::N;
    const int64_t mis = (int64_t)((uintptr_t)V & 15u);
    vec = n >= 4 * VEC && mis % (int64_t)sizeof(T) == 0 && (k <= 1 || ldv % VEC == 0);
    head = vec && mis ? (16 - mis) / (int64_t)sizeof(T) : 0;
    nvec = vec ? (n - head) / VEC : n;
  }
  bool same_phase(const T *p) const { return vec && (((uintptr_t)(p + head)) & 15u) == 0; }
};

inline int kry_grid(const mxlo_ctx *ctx, int64_t nvec, int64_t per_block) {
  const int g = grid_for(ctx, nvec, per_block, ctx->tune.red_blocks_per_cu > 0 ? ctx->tune.red_blocks_per_cu : 4);
  return g > kMaxRedBlocks ? kMaxRedBlocks : g;
}

template <int NC>
constexpr int kry_unroll() { return NC <= 2 ? 4 : (NC <= 5 ? 2 : 1); }

// one group of nc columns: dots (update == false) or update
template <typename T, bool UPDATE>
int32_t korth_group(mxlo_ctx *ctx, const Walk<T> &wk, const T *Vg, int64_t ldv, int nc, T *w, int64_t n, bool nt,
                    const double *h, int first, int last, const double *skip, int *grid_out) {
  constexpr int VEC = Vec16<T>::N;
  const bool wvec = wk.same_phase(w);
  with_nc(nc, [&]<int NC>() {
    constexpr int UNROLL = kry_unroll<NC>();
    const int grid = kry_grid(ctx, wk.nvec, (int64_t)kBlock * UNROLL);
    *grid_out = grid;
    auto go = [&]<int VECV, bool WVEC, bool NT>() {
      if constexpr (UPDATE)
        hipLaunchKernelGGL((korth_update_kernel<T, VECV, NC, UNROLL, WVEC, NT>), dim3(grid), dim3(kBlock), 0, ctx->stream, Vg, ldv,
                           w, wk.head, wk.nvec, n, h, ctx->partials, first, last, skip);
      else
        hipLaunchKernelGGL((korth_dots_kernel<T, VECV, NC, UNROLL, WVEC, NT>), dim3(grid), dim3(kBlock), 0, ctx->stream, Vg, ldv,
                           (const T *)w, wk.head, wk.nvec, n, ctx->partials, skip);
    };
    if constexpr (NC <= kKryNCScalar) {
      if (!wk.vec) {
        go.template operator()<1, false, false>();
        return;
      }
    }
    if (wvec && nt) go.template operator()<VEC, true, true>();
    else if (wvec) go.template operator()<VEC, true, false>();
    else if (nt) go.template operator()<VEC, false, true>();
    else go.template operator()<VEC, false, false>();
  });
  MXLO_LAUNCH_CHECK();
  return MXLO_OK;
}

template <typename T>
int32_t normalise(mxlo_ctx *ctx, T *x, int64_t n, const double *beta) {
  constexpr int VEC = Vec16<T>::N;
  const Walk<T> wk(x, n, 1, n);
  const int grid = kry_grid(ctx, wk.nvec, kBlock);
  if (wk.vec)
    hipLaunchKernelGGL((kry_normalise_kernel<T, VEC>), dim3(grid), dim3(kBlock), 0, ctx->stream, x, wk.head, wk.nvec, n, beta);
  else
    hipLaunchKernelGGL((kry_normalise_kernel<T, 1>), dim3(grid), dim3(kBlock), 0, ctx->stream, x, (int64_t)0, n, n, beta);
  MXLO_LAUNCH_CHECK();
  return MXLO_OK;
}

template <typename T>
int32_t krylov_orth_t(mxlo_ctx *ctx, const T *V, int64_t ldv, int64_t n, int k, T *w, double *coef, bool dgks) {
  double *ws = ctx->scalars + kKryScalars;
  const Walk<T> wk(V, ldv, k, n);
  const bool nt = (int64_t)sizeof(T) * n * (k + 1) >= ctx->tune.nt_min_bytes;
  const int gmax = wk.vec ? kKryNC : kKryNCScalar;
  for (int round = 1; round <= 2; ++round) {
    const double *skip = (round == 2 && dgks) ? ws + kKrySkip : nullptr;
    int grid = 0, grid_first = 0;
    for (int c0 = 0; c0 < k; c0 += gmax) {   // h = V'w, group by group; w is not touched until every group is done
      const int nc = k - c0 < gmax ? k - c0 : gmax;
      MXLO_TRY((korth_group<T, false>(ctx, wk, V + (int64_t)c0 * ldv, ldv, nc, w, n, nt, nullptr, 0, 0, skip, &grid)));
      hipLaunchKernelGGL(kry_finalize_kernel, dim3(nc), dim3(kBlock), 0, ctx->stream, ctx->partials, grid, ws + c0, skip, 0);
      MXLO_LAUNCH_CHECK();
    }
    for (int c0 = 0; c0 < k; c0 += gmax) {   // w -= V h; the first group leaves sum w_old^2 in row 0, the last sum w_new^2 in row 1
      const int nc = k - c0 < gmax ? k - c0 : gmax;
      MXLO_TRY((korth_group<T, true>(ctx, wk, V + (int64_t)c0 * ldv, ldv, nc, w, n, nt, ws + c0, c0 == 0, c0 + nc == k, skip,
                                     &grid)));
      if (c0 == 0) grid_first = grid;
    }
    // a short last group runs with another unroll factor, hence another grid: each row is summed over its own launch's
    hipLaunchKernelGGL(korth_finish_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, ctx->partials, grid_first, grid, ws, k, coef,
                       round, skip);
    MXLO_LAUNCH_CHECK();
  }
  return normalise<T>(ctx, w, n, coef + k);
}

template <typename T>
int32_t krylov_combine_t(mxlo_ctx *ctx, const T *V, int64_t ldv, int64_t n, int k, const double *y, T *out, double *coef) {
  constexpr int VEC = Vec16<T>::N;
  const Walk<T> wk(V, ldv, k, n);
  const bool ovec = wk.same_phase(out);
  const bool nt = (int64_t)sizeof(T) * n * (k + 1) >= ctx->tune.nt_min_bytes;
  const int grid = kry_grid(ctx, wk.nvec, kBlock);
  auto go = [&]<int VECV, bool OVEC, bool NT>() {
    hipLaunchKernelGGL((kry_combine_kernel<T, VECV, OVEC, NT>), dim3(grid), dim3(kBlock), 0, ctx->stream, V, ldv, k, y, out,
                       wk.head, wk.nvec, n, ctx->partials);
  };
  if (!wk.vec) go.template operator()<1, false, false>();
  else if (ovec && nt) go.template operator()<VEC, true, true>();
  else if (ovec) go.template operator()<VEC, true, false>();
  else if (nt) go.template operator()<VEC, false, true>();
  else go.template operator()<VEC, false, false>();
  MXLO_LAUNCH_CHECK();
  hipLaunchKernelGGL(kry_finalize_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, ctx->partials, grid, coef, (const double *)nullptr, 1);
  MXLO_LAUNCH_CHECK();
  return normalise<T>(ctx, out, n, coef);
}

int32_t krylov_common(mxlo_ctx *ctx, int32_t dtype, const void *V, int64_t ldv, int64_t n, int32_t k, const void *x,
                      const void *p1, const void *p2, const char *name) {
  MXLO_REQUIRE(ctx != nullptr, MXLO_EINVAL, "%s: ctx is NULL", name);
  MXLO_REQUIRE(dtype == MXLO_F64 || dtype == MXLO_F32, MXLO_EINVAL, "%s: bad dtype %d (real f64 / f32 only)", name, dtype);
  MXLO_REQUIRE(!ctx->allreduce, MXLO_ESTATE,
               "%s: the ctx has an all-reduce hook installed — row-sharded bases are not supported", name);
  MXLO_REQUIRE(n >= 1 && k >= 1 && k <= kKryMaxK && ldv >= n && V && x && p1 && p2, MXLO_EINVAL,
               "%s: bad argument (n = %lld, k = %d of at most %d, ldv = %lld)", name, (long long)n, k, kKryMaxK, (long long)ldv);
  const uintptr_t es = dtype == MXLO_F64 ? 8 : 4;
  MXLO_REQUIRE((uintptr_t)V % es == 0 && (uintptr_t)x % es == 0 && ((uintptr_t)p1 | (uintptr_t)p2) % 8 == 0, MXLO_EINVAL,
               "%s: operands must be aligned to their element size", name);
  return MXLO_OK;
}

}  // namespace

}  // namespace mxlo

using namespace mxlo;

MXLO_API int32_t mxlo_krylov_orth(mxlo_ctx *ctx, int32_t dtype, const void *V, int64_t ldv, int64_t n, int32_t k, void *w,
                                  double *coef, int32_t flags) {
  MXLO_TRY(krylov_common(ctx, dtype, V, ldv, n, k, w, coef, coef, "mxlo_krylov_orth"));
  MXLO_REQUIRE((flags & ~MXLO_KRYLOV_DGKS) == 0, MXLO_EINVAL, "mxlo_krylov_orth: unknown flags 0x%x", flags);
  const int64_t es = dtype == MXLO_F64 ? 8 : 4;
  MXLO_REQUIRE(!bytes_overlap(V, ((int64_t)(k - 1) * ldv + n) * es, w, n * es), MXLO_EINVAL,
               "mxlo_krylov_orth: w overlaps the first %d columns of V", k);
  MXLO_DEVICE_GUARD(ctx);
  const bool dgks = (flags & MXLO_KRYLOV_DGKS) != 0;
  if (dtype == MXLO_F64) return krylov_orth_t<double>(ctx, (const double *)V, ldv, n, k, (double *)w, coef, dgks);
  return krylov_orth_t<float>(ctx, (const float *)V, ldv, n, k, (float *)w, coef, dgks);
}

MXLO_API int32_t mxlo_krylov_combine(mxlo_ctx *ctx, int32_t dtype, const void *V, int64_t ldv, int64_t n, int32_t k,
                                     const double *y_dev, void *out, double *coef) {
  MXLO_TRY(krylov_common(ctx, dtype, V, ldv, n, k, out, y_dev, coef, "mxlo_krylov_combine"));
  const int64_t es = dtype == MXLO_F64 ? 8 : 4;
  if (bytes_overlap(V, ((int64_t)(k - 1) * ldv + n) * es, out, n * es)) {
    // out inside the basis: only as one of its columns — element i of out is then element i of that column, read and
    // written by the same lane, in that order
    const int64_t d = (int64_t)((const char *)out - (const char *)V);
    MXLO_REQUIRE(d >= 0 && d % (ldv * es) == 0, MXLO_EINVAL,
                 "mxlo_krylov_combine: out overlaps V without being one of its columns");
  }
  MXLO_DEVICE_GUARD(ctx);
  if (dtype == MXLO_F64) return krylov_combine_t<double>(ctx, (const double *)V, ldv, n, k, y_dev, (double *)out, coef);
  return krylov_combine_t<float>(ctx, (const float *)V, ldv, n, k, y_dev, (float *)out, coef);
}
