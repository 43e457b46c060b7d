// linalg.hip — opCholesky, opLDL (dense), opLU and triangular opInverse (src/linalg.jl:3-9, 27-32, 44-58, 60-75): the factorisations, the
// inverses of the diagonal blocks and the block substitution sweeps. Everything is cut into block columns of NB = 64.
//
// The only dependency mechanism is the LAUNCH BOUNDARY: no workgroup waits for another one. A sweep is a chain of launches,
// one per block column (block row for a transposed solve). In launch k every workgroup reads the solved block x_k (64
// doubles, finished by the launch before) and subtracts its 64 x 64 piece of the panel from the right-hand side; the ONE
// workgroup whose 64 entries are the next diagonal block goes on and solves it, x_{k+1} = inv(T_{k+1,k+1}) b_{k+1}, with the
// stored inverse. The right-hand side lives in one f64 work vector z whose blocks turn into the solution one by one, so the
// data a launch reads (x_k) and writes (entries not solved yet) never meet. All sums run in a fixed order in f64.
// Matrix operands (the mxlo_*_mul_block entry points) run the same chain with up to KB = 8 right-hand sides per launch.
#include "common.h"

using namespace mxlo;

namespace {

constexpr int NB = 64;               // block column width; one diagonal block (f64) is 32 KiB of LDS
constexpr int NB2 = NB * NB;

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ double ld_stream(const T *p) {   // the triangle is read once per sweep: do not keep it in cache
  return (double)__builtin_nontemporal_load(p);
}

// ---------------------------------------------------------------------------------------------- triangularity
// bit 0: the strict upper triangle holds a non-zero (NaN counts), bit 1: the strict lower one does
template <typename T>
__global__ void __launch_bounds__(kBlock) tri_kind_kernel(const T *__restrict__ M, int64_t ld, int64_t n, int *flag) {
  int f = 0;
  for (int64_t c = blockIdx.x; c < n; c += gridDim.x)
    for (int64_t i = threadIdx.x; i < n; i += kBlock) {
      const T x = M[i + c * ld];
      if (x != T(0)) f |= i < c ? 1 : (i > c ? 2 : 0);
    }
  const int up = __syncthreads_or(f & 1), lo = __syncthreads_or(f & 2);
  if (threadIdx.x == 0 && (up || lo)) atomicOr(flag, (up ? 1 : 0) | (lo ? 2 : 0));
}

// ---------------------------------------------------------------------------------------------- 64 x 64 blocks in LDS
// Blocks are stored column-major without padding, s[c * NB + i]; a wave's lanes are the ROWS i (conflict-free), its wave
// index q picks the columns c = q, q + 4, ... A block narrower than NB is padded with the identity.

// Cholesky of the lower triangle held in sA; the factor goes to sL (zero above the diagonal). Returns 0, or the 1-based
// index of the first pivot that is not positive and finite (the same value in every thread).
__device__ int chol_block(double *sA, double *sL, int lane, int q) {
  for (int p = 0; p < NB; ++p) {
    const double app = sA[p * NB + p];
    if (!(app > 0.0) || !(app < __builtin_inf())) return p + 1;
    const double lpp = sqrt(app);
    if (q == 0) sL[p * NB + lane] = lane > p ? sA[p * NB + lane] / lpp : (lane == p ? lpp : 0.0);
    __syncthreads();
    const double lip = sL[p * NB + lane];
#pragma unroll 4
    for (int c = q; c < NB; c += 4)
      if (c > p && lane >= c) sA[c * NB + lane] = fma(-lip, sL[p * NB + c], sA[c * NB + lane]);
    __syncthreads();
  }
  return 0;
}

// Unpivoted LDL' of the lower triangle held in sA, in place: sA becomes Lt = L D (the pivots d on its diagonal, column c of
// the unit L times d_c below it) — right-looking elimination that never scales a column. Returns 0, or the 1-based index
// of the first pivot that is zero or not finite (the same value in every thread). Negative and tiny pivots are taken.
__device__ int ldlt_block(double *sA, int lane, int q) {
  for (int p = 0; p < NB; ++p) {
    const double dp = sA[p * NB + p];
    if (dp == 0.0 || !(fabs(dp) < __builtin_inf())) return p + 1;
    const double lip = sA[p * NB + lane] / dp;
#pragma unroll 4
    for (int c = q; c < NB; c += 4)
      if (c > p && lane >= c) sA[c * NB + lane] = fma(-lip, sA[p * NB + c], sA[c * NB + lane]);
    __syncthreads();
  }
  return 0;
}

// sX = inv(sL) for a lower triangular sL: forward substitution on the identity, all 64 columns at once.
__device__ void invert_block(const double *sL, double *sX, int tid, int lane, int q) {
  for (int e = tid; e < NB2; e += kBlock) sX[e] = (e >> 6) == (e & 63) ? 1.0 : 0.0;
  __syncthreads();
  for (int p = 0; p < NB; ++p) {
    if (tid < NB) sX[tid * NB + p] = sX[tid * NB + p] / sL[p * NB + p];     // row p of the inverse is final
    __syncthreads();
    const double lip = sL[p * NB + lane];
#pragma unroll 4
    for (int c = q; c < NB; c += 4)
      if (lane > p) sX[c * NB + lane] = fma(-lip, sX[c * NB + p], sX[c * NB + lane]);
    __syncthreads();
  }
}

// inverses of ALL diagonal blocks of a triangular matrix, one workgroup each (opInverse). An upper block is inverted as the
// lower block that is its transpose and stored transposed back.
template <typename T>
__global__ void __launch_bounds__(kBlock) tri_prepare_kernel(const T *__restrict__ Tm, int64_t ld, int64_t n, int upper,
                                                             double *__restrict__ dinv) {
  __shared__ double sL[NB2], sX[NB2];
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int64_t j0 = (int64_t)blockIdx.x * NB;
  const int jb = (int)(n - j0 < NB ? n - j0 : NB);
  for (int c = q; c < NB; c += 4) {
    double x = lane == c ? 1.0 : 0.0;
    if (lane >= c && lane < jb) x = (double)(upper ? Tm[(j0 + c) + (j0 + lane) * ld] : Tm[(j0 + lane) + (j0 + c) * ld]);
    sL[c * NB + lane] = x;
  }
  __syncthreads();
  invert_block(sL, sX, tid, lane, q);
  double *out = dinv + (int64_t)blockIdx.x * NB2;
  for (int c = q; c < NB; c += 4) out[upper ? lane * NB + c : c * NB + lane] = sX[c * NB + lane];
}

// ---------------------------------------------------------------------------------------------- potrf
// W (lower triangle, column-major) = the UPPER triangle of M, transposed: W[i, c] = M[c, i], i >= c.
template <typename T>
__global__ void __launch_bounds__(kBlock) pack_upper_kernel(T *__restrict__ W, int64_t ldw, const T *__restrict__ M, int64_t ldm,
                                                            int rowmajor, int64_t n) {
  if (blockIdx.y > blockIdx.x) return;                 // tile (bi, bc) of W with bi >= bc
  __shared__ T s[NB * (NB + 1)];
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * NB, c0 = (int64_t)blockIdx.y * NB;
  if (rowmajor) {                                      // M[c, i] = M[c * ldm + i]: unit stride along i, as W wants it
    for (int cl = q; cl < NB; cl += 4) {
      const int64_t i = i0 + lane, c = c0 + cl;
      if (i < n && c < n) W[i + c * ldw] = i >= c ? M[c * ldm + i] : T(0);
    }
    return;
  }
  for (int il = q; il < NB; il += 4) {                 // M[c, i] = M[c + i * ldm]: unit stride along c, transposed through LDS
    const int64_t i = i0 + il, c = c0 + lane;
    s[il * (NB + 1) + lane] = (i < n && c < n && i >= c) ? M[c + i * ldm] : T(0);
  }
  __syncthreads();
  for (int cl = q; cl < NB; cl += 4) {
    const int64_t i = i0 + lane, c = c0 + cl;
    if (i < n && c < n) W[i + c * ldw] = s[lane * (NB + 1) + cl];
  }
}

// phase (a): factor the diagonal block, store its explicit inverse
template <typename T>
__global__ void __launch_bounds__(kBlock) potrf_diag_kernel(T *__restrict__ W, int64_t ldw, int64_t n, int64_t j0,
                                                            double *__restrict__ dinv, int *info) {
  __shared__ double sA[NB2], sL[NB2];
  if (*info != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int jb = (int)(n - j0 < NB ? n - j0 : NB);
  for (int c = q; c < NB; c += 4) {
    double x = lane == c ? 1.0 : 0.0;
    if (lane >= c && lane < jb) x = (double)W[(j0 + lane) + (j0 + c) * ldw];
    sA[c * NB + lane] = x;
  }
  __syncthreads();
  const int bad = chol_block(sA, sL, lane, q);
  if (bad) {
    if (tid == 0) *info = (int)(j0 + bad);
    return;
  }
  for (int c = q; c < NB; c += 4)
    if (lane >= c && lane < jb) W[(j0 + lane) + (j0 + c) * ldw] = (T)sL[c * NB + lane];
  invert_block(sL, sA, tid, lane, q);
  for (int e = tid; e < NB2; e += kBlock) dinv[e] = sA[e];
}

// phase (a) of mxlo_ldlt: M_kk = L_kk D_k L_kk'. The block keeps Lt_kk = L_kk D_k, d gets the pivots, dinv the inverse of Lt_kk
template <typename T>
__global__ void __launch_bounds__(kBlock) ldlt_diag_kernel(T *__restrict__ W, int64_t ldw, int64_t n, int64_t j0,
                                                           double *__restrict__ dinv, double *__restrict__ d, int *info) {
  __shared__ double sA[NB2], sX[NB2];
  if (*info != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int jb = (int)(n - j0 < NB ? n - j0 : NB);
  for (int c = q; c < NB; c += 4) {
    double x = lane == c ? 1.0 : 0.0;
    if (lane >= c && lane < jb) x = (double)W[(j0 + lane) + (j0 + c) * ldw];
    sA[c * NB + lane] = x;
  }
  __syncthreads();
  const int bad = ldlt_block(sA, lane, q);
  if (bad) {
    if (tid == 0) *info = (int)(j0 + bad);
    return;
  }
  for (int c = q; c < NB; c += 4)
    if (lane >= c && lane < jb) W[(j0 + lane) + (j0 + c) * ldw] = (T)sA[c * NB + lane];
  if (tid < jb) d[j0 + tid] = sA[tid * NB + tid];
  invert_block(sA, sX, tid, lane, q);
  for (int e = tid; e < NB2; e += kBlock) dinv[e] = sX[e];
}

// phase (b): the panel below the diagonal block, W[i, j0 + c] = sum_{p <= c} W[i, j0 + p] inv(L_kk)[c, p], 64 rows a workgroup.
// LDL: dinv is inv(Lt_kk) = inv(D_k) inv(L_kk), so the sum is the panel of the unit L; times d_c it is the panel of Lt = L D.
template <typename T, bool LDL>
__global__ void __launch_bounds__(kBlock) potrf_panel_kernel(T *__restrict__ W, int64_t ldw, int64_t n, int64_t j0, int jb,
                                                             const double *__restrict__ dinv, const double *__restrict__ d,
                                                             const int *info) {
  __shared__ double sP[NB2], sD[NB2];
  if (*info != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int64_t i = j0 + jb + (int64_t)blockIdx.x * NB + lane;
  for (int e = tid; e < NB2; e += kBlock) sD[e] = dinv[e];
  for (int p = q; p < NB; p += 4) sP[p * NB + lane] = (p < jb && i < n) ? (double)W[i + (j0 + p) * ldw] : 0.0;
  __syncthreads();
  for (int c = q; c < jb; c += 4) {
    double acc = 0.0;
    for (int p = 0; p <= c; ++p) acc = fma(sP[p * NB + lane], sD[p * NB + c], acc);
    if constexpr (LDL) acc *= d[j0 + c];
    if (i < n) W[i + (j0 + c) * ldw] = (T)acc;
  }
}

// phase (c): C -= P P' on the lower triangle of the trailing matrix; 64 x 64 tiles, the ones above the diagonal are skipped.
// LDL: C -= (P inv(D_k)) P' with P the panel of Lt; the column scaling 1 / d is applied while the row operand is staged.
// v_mfma_f64_16x16x4_f64: C/D row = (lane >> 4) + 4 reg, col = lane & 15; the f32 form has row = 4 (lane >> 4) + reg.
template <typename T>
struct Mfma;
template <>
struct Mfma<double> {
  using Acc = f64x4;
  static __device__ __forceinline__ Acc run(double a, double b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) + 4 * r; }
};
template <>
struct Mfma<float> {
  using Acc = f32x4v;
  static __device__ __forceinline__ Acc run(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int row(int lane, int r) { return 4 * (lane >> 4) + r; }
};

constexpr int SK = 16, SLD = 80;     // k-slab and padded LDS row of the SYRK tiles (dense.hip's gemm_kernel uses the same)

template <typename T, bool LDL>
__global__ void __launch_bounds__(kBlock) potrf_syrk_kernel(T *__restrict__ C, const T *__restrict__ P, int64_t ld, int M, int K,
                                                            const double *__restrict__ d, const int *info) {
  if (blockIdx.y > blockIdx.x) return;
  if (*info != 0) return;
  __shared__ T sA[SK][SLD], sB[SK][SLD];
  __shared__ T sR[LDL ? NB : 1];                         // 1 / d of this block column (K <= NB)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if constexpr (LDL) {
    if (tid < NB) sR[tid] = tid < K ? (T)(1.0 / d[tid]) : T(0);
    __syncthreads();
  }
  const int bm = blockIdx.x * NB, bn = blockIdx.y * NB;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  using Acc = typename Mfma<T>::Acc;
  Acc acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[a][b][r] = 0;
  for (int k0 = 0; k0 < K; k0 += SK) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int e = tid + t * kBlock, i = e & 63, k = e >> 6, gk = k0 + k;
      T pa = (bm + i < M && gk < K) ? P[(bm + i) + (int64_t)gk * ld] : T(0);
      if constexpr (LDL) pa *= sR[gk & (NB - 1)];
      sA[k][i] = pa;
      sB[k][i] = (bn + i < M && gk < K) ? P[(bn + i) + (int64_t)gk * ld] : T(0);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < SK; kk += 4) {
      const int kr = kk + (lane >> 4);
      const T a0 = sA[kr][wm + (lane & 15)], a1 = sA[kr][wm + 16 + (lane & 15)];
      const T b0 = sB[kr][wn + (lane & 15)], b1 = sB[kr][wn + 16 + (lane & 15)];
      acc[0][0] = Mfma<T>::run(a0, b0, acc[0][0]);
      acc[0][1] = Mfma<T>::run(a0, b1, acc[0][1]);
      acc[1][0] = Mfma<T>::run(a1, b0, acc[1][0]);
      acc[1][1] = Mfma<T>::run(a1, b1, acc[1][1]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = bm + wm + a * 16 + Mfma<T>::row(lane, r), gj = bn + wn + b * 16 + (lane & 15);
        if (gi < M && gj <= gi) {
          T *p = C + gi + (int64_t)gj * ld;
          *p = *p - acc[a][b][r];
        }
      }
}

// ---------------------------------------------------------------------------------------------- getrf
// P A = L U with partial pivoting, right-looking in block columns of NB. Per block column: (a) ONE workgroup factors the
// whole panel (all rows below, in global memory: the panel of a large matrix does not fit a CU), searching each pivot
// over the full remaining height, so the data-dependent decision never leaves the device and the chain of launches
// depends on n only; (b) the inverses of both triangles of the diagonal block; (c) the panel's interchanges applied to
// the columns left and right of it; (d) U12 = inv(L11) A12; (e) A22 -= L21 U12 on MFMA.
constexpr int PT = 1024;             // threads of the panel workgroup: 16 waves hide the latency of one CU's loads

// is the candidate (|a|, ia) a better pivot than (|b|, ib)? The larger one, a NaN before any number, the first row on a tie
__device__ __forceinline__ bool pivot_better(double a, int ia, double b, int ib) {
  const bool an = a != a, bn = b != b;
  if (an || bn) return an && (!bn || ia < ib);
  return a > b || (a == b && ia < ib);
}

// W = M and perm = ipiv = 0 .. n - 1 (M == NULL: only the latter)
template <typename T>
__global__ void __launch_bounds__(kBlock) getrf_copy_kernel(T *__restrict__ W, int64_t ldw, const T *__restrict__ M, int64_t ldm,
                                                            int64_t n, int *__restrict__ perm) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  if (blockIdx.y == 0) perm[i] = perm[n + i] = (int)i;
  if (M)
    for (int64_t c = blockIdx.y; c < n; c += gridDim.y) W[i + c * ldw] = M[i + c * ldm];
}

// phase (a): columns j0 .. j0 + jb of rows j0 .. n. For each column: the pivot search, the interchange inside the panel,
// the multipliers (f64 quotient, stored in T) and the rank-1 update of the panel's remaining columns.
template <typename T>
__global__ void __launch_bounds__(PT) getrf_panel_kernel(T *W, int64_t ldw, int64_t n, int64_t j0, int jb, int *perm, int *info) {
  __shared__ double s_val[PT / 64], s_u[NB], s_pv;
  __shared__ int s_idx[PT / 64], s_row, s_bad;
  if (*info != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int *ipiv = perm + n;
  for (int p = 0; p < jb; ++p) {
    const int64_t jp = j0 + p;
    T *col = W + jp * ldw;
    double best = -1.0;                                  // below every |a|: the first candidate is always taken
    int bi = 0x7fffffff;
    for (int64_t i = jp + tid; i < n; i += PT) {
      const double a = fabs((double)col[i]);
      if (!(a <= best) && best == best) { best = a; bi = (int)i; }      // a NaN is taken and then kept
    }
    for (int o = 32; o; o >>= 1) {
      const double ob = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (pivot_better(ob, oi, best, bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) { s_val[wave] = best; s_idx[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < PT / 64; ++w)
        if (pivot_better(s_val[w], s_idx[w], best, bi)) { best = s_val[w]; bi = s_idx[w]; }
      const double pv = (double)col[bi];
      const int bad = pv == 0.0 || !(fabs(pv) < __builtin_inf());
      if (bad) *info = (int)(jp + 1);
      else {
        ipiv[jp] = bi;
        const int t = perm[jp];
        perm[jp] = perm[bi];
        perm[bi] = t;
      }
      s_row = bi; s_pv = pv; s_bad = bad;
    }
    __syncthreads();
    if (s_bad) return;
    const int64_t r = s_row;
    const double pv = s_pv;
    if (tid < jb) {                                      // rows jp and r change places inside the panel; row p of U to LDS
      T *c = W + (j0 + tid) * ldw;
      const T x = c[r];
      if (r != jp) { c[r] = c[jp]; c[jp] = x; }
      s_u[tid] = (double)x;
    }
    __syncthreads();
    const int64_t rows = n - jp - 1, rch = (rows + 63) / 64;
    for (int64_t rc = wave; rc < rch; rc += PT / 64) {    // 64 rows a wave: the multiplier, then its row of the update
      const int64_t i = jp + 1 + rc * 64 + lane;
      if (i < n) {
        const T lt = (T)((double)col[i] / pv);
        col[i] = lt;
        const double l = (double)lt;
        for (int c = p + 1; c < jb; ++c) {
          T *e = W + i + (j0 + c) * ldw;
          *e = (T)fma(-l, s_u[c], (double)*e);
        }
      }
    }
    __syncthreads();
  }
}

// phase (b): inv(L11) of the unit lower triangle (workgroup 0) and inv(U11) (workgroup 1) of the factored diagonal block;
// the upper one is inverted as its transpose, as in tri_prepare_kernel
template <typename T>
__global__ void __launch_bounds__(kBlock) getrf_inv_kernel(const T *__restrict__ W, int64_t ldw, int64_t n, int64_t j0,
                                                           double *__restrict__ dl, double *__restrict__ du, const int *info) {
  __shared__ double sL[NB2], sX[NB2];
  if (*info != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int upper = blockIdx.x;
  const int jb = (int)(n - j0 < NB ? n - j0 : NB);
  for (int c = q; c < NB; c += 4) {
    double x = lane == c ? 1.0 : 0.0;
    if (lane < jb) {
      if (upper && lane >= c) x = (double)W[(j0 + c) + (j0 + lane) * ldw];
      if (!upper && lane > c) x = (double)W[(j0 + lane) + (j0 + c) * ldw];
    }
    sL[c * NB + lane] = x;
  }
  __syncthreads();
  invert_block(sL, sX, tid, lane, q);
  double *out = upper ? du : dl;
  for (int c = q; c < NB; c += 4) out[upper ? lane * NB + c : c * NB + lane] = sX[c * NB + lane];
}

// phase (c): the panel's jb interchanges, in order, on every column outside the panel; one thread a column
template <typename T>
__global__ void __launch_bounds__(kBlock) getrf_swap_kernel(T *W, int64_t ldw, int64_t n, int64_t j0, int jb, const int *perm,
                                                            const int *info) {
  __shared__ int sp[NB];
  if (*info != 0) return;
  if (threadIdx.x < jb) sp[threadIdx.x] = perm[n + j0 + threadIdx.x];
  __syncthreads();
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n - jb) return;
  T *col = W + (idx < j0 ? idx : idx + jb) * ldw;
  for (int p = 0; p < jb; ++p) {
    const int64_t r = sp[p];
    if (r != j0 + p) {
      const T x = col[j0 + p];
      col[j0 + p] = col[r];
      col[r] = x;
    }
  }
}

// phase (d): U12 = inv(L11) A12 with the stored inverse, 64 columns a workgroup, the lanes down the rows
template <typename T>
__global__ void __launch_bounds__(kBlock) getrf_row_kernel(T *__restrict__ W, int64_t ldw, int64_t n, int64_t j0, int jb,
                                                           const double *__restrict__ dinv, const int *info) {
  __shared__ double sP[NB2], sD[NB2];
  if (*info != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int64_t c0 = j0 + jb + (int64_t)blockIdx.x * NB;
  for (int e = tid; e < NB2; e += kBlock) sD[e] = dinv[e];
  for (int c = q; c < NB; c += 4) sP[c * NB + lane] = (lane < jb && c0 + c < n) ? (double)W[(j0 + lane) + (c0 + c) * ldw] : 0.0;
  __syncthreads();
  for (int c = q; c < NB; c += 4) {
    double acc = 0.0;
    for (int p = 0; p < jb; ++p) {
      const double t = fma(sD[p * NB + lane], sP[c * NB + p], acc);
      acc = p <= lane ? t : acc;
    }
    if (lane < jb && c0 + c < n) W[(j0 + lane) + (c0 + c) * ldw] = (T)acc;
  }
}

// phase (e): C -= A B, C the M x M trailing matrix, A = L21 (M x K, column-major) and B = U12 (K x M): potrf_syrk_kernel with
// two different operands and every tile
template <typename T>
__global__ void __launch_bounds__(kBlock) getrf_gemm_kernel(T *__restrict__ C, const T *__restrict__ A, const T *__restrict__ B,
                                                            int64_t ld, int M, int K, const int *info) {
  if (*info != 0) return;
  __shared__ T sA[SK][SLD], sB[SK][SLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bm = blockIdx.x * NB, bn = blockIdx.y * NB;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  using Acc = typename Mfma<T>::Acc;
  Acc acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[a][b][r] = 0;
  for (int k0 = 0; k0 < K; k0 += SK) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int e = tid + t * kBlock, i = e & 63, k = e >> 6, kb = e & 15, jn = e >> 4;
      sA[k][i] = (bm + i < M && k0 + k < K) ? A[(bm + i) + (int64_t)(k0 + k) * ld] : T(0);
      sB[kb][jn] = (bn + jn < M && k0 + kb < K) ? B[(k0 + kb) + (int64_t)(bn + jn) * ld] : T(0);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < SK; kk += 4) {
      const int kr = kk + (lane >> 4);
      const T a0 = sA[kr][wm + (lane & 15)], a1 = sA[kr][wm + 16 + (lane & 15)];
      const T b0 = sB[kr][wn + (lane & 15)], b1 = sB[kr][wn + 16 + (lane & 15)];
      acc[0][0] = Mfma<T>::run(a0, b0, acc[0][0]);
      acc[0][1] = Mfma<T>::run(a0, b1, acc[0][1]);
      acc[1][0] = Mfma<T>::run(a1, b0, acc[1][0]);
      acc[1][1] = Mfma<T>::run(a1, b1, acc[1][1]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = bm + wm + a * 16 + Mfma<T>::row(lane, r), gj = bn + wn + b * 16 + (lane & 15);
        if (gi < M && gj < M) {
          T *p = C + gi + (int64_t)gj * ld;
          *p = *p - acc[a][b][r];
        }
      }
}

// ---------------------------------------------------------------------------------------------- substitution sweeps
struct SweepArgs {
  const void *Tm;        // the triangle, column-major
  int64_t ld, n;
  double *z;             // right-hand side turning into the solution, block by block
  const void *v;         // first launch of an apply: the right-hand side is read from v (no panel yet), else NULL
  int64_t xs;            // the solved block is x = z[xs .. xs + xl); xl == 0: no panel
  int xl;
  int64_t r0, r1;        // entries this launch updates, in chunks of NB from r0
  int nchunks;
  int rowpanel;          // 0: z[i] -= sum_c T[i, xs + c] x[c]      1: z[c] -= sum_i T[xs + i, c] x[i]
  int gd;                // the chunk that is the next diagonal block (-1: none) ...
  const double *dinv;    // ... its stored inverse, applied transposed if dinv_t
  int dinv_t;
  const double *dinv2;   // turn-around: a second product, with this block (Cholesky: the same one), transposed if dinv2_t, or NULL
  int dinv2_t;
  int epi;               // last launch: res = alpha x + beta res — chunk gd for its own block, the further workgroups for the rest
  void *res;
  double alpha, beta;
  const double *dsc;     // opLDL: the pivots d. The turn-around block is multiplied by them between its two products, and ...
  int zscale;            // ... in the first launch of the back sweep every right-hand side block is, as it is read
  const int *gather;     // opLU: entry i of the right-hand side is v[gather[i]] (first launch), or NULL
  const int *scatter;    // opLU: the epilogue writes entry i of the solution to res[scatter[i]], or NULL
  int tri_upper;         // the diagonal block as the triangle stores it: in its upper part (else the lower one) ...
  int tri_unit;          // ... with an implicit unit diagonal (opLU's L); read by the refinement step of the block solve
  int tri2_upper;        // the same for the block of the turn-around product
  int tri2_unit;
  int kb;                // block form (sweep_block_kernel): the group's right-hand sides, 1 .. KB; 0: the vector kernel. v and res
  int64_t ldr, ldv;      // are then n x kb matrices with these leading dimensions, z is n x kb with column stride n
  double *xacc;          // refined apply (block form only), else NULL: the iterate x, n x kb f64 with column stride n, in the sweep's own
  int xmode;             // order. The launch with epi does — 1: x = z   2: x += z   3: res = alpha (x + z) + beta res (scattered); res is
};                       // touched by 3 only


__device__ __forceinline__ double block_gemv(const double *__restrict__ D, bool trans, const double *sb, double (*spart)[NB],
                                             int lane, int q) {
  double part = 0.0;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int c = q * 16 + t;
    part = fma(trans ? D[lane * NB + c] : D[c * NB + lane], sb[c], part);
  }
  spart[q][lane] = part;
  __syncthreads();
  const double x = (spart[0][lane] + spart[1][lane]) + (spart[2][lane] + spart[3][lane]);
  __syncthreads();
  return x;
}

// One step of iterative refinement of a block solve, x += inv(M) (b - M x), all in f64. M = S or S' (trans) is the diagonal
// block, S read from the triangle itself (blk, its valid part only; unit: an implicit 1 on the diagonal), inv(M) the stored
// inverse D (applied transposed if trans). The product with an explicit inverse alone has a residual of the order of
// eps |M| |inv(M)| |b|, which on an ill-conditioned block is far from backward stable; the inverse computed column by column
// has a small right residual |M X - I| <= gamma |M| |X|, so one step brings the residual down to the size substitution
// leaves, eps (|M| |x| + |b|). b is in sb, rows past cl hold b = x = 0. sx is scratch; every thread returns x of row `lane`.
template <typename T>
__device__ __forceinline__ double block_refine(const T *__restrict__ blk, int64_t ld, int cl, bool trans, bool upper, bool unit,
                                               const double *__restrict__ D, double x, const double *sb, double *sx,
                                               double (*spart)[NB], int tid, int lane, int q) {
  if (tid < NB) sx[tid] = x;
  __syncthreads();
  double part = 0.0;
  if (lane < cl) {
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int c = q * 16 + t;
      if (c < cl) {
        const int r = trans ? c : lane, s = trans ? lane : c;              // M[lane, c] = S[r, s]
        double m = 0.0;
        if (r == s && unit) m = 1.0;
        else if (upper ? r <= s : r >= s) m = (double)blk[r + (int64_t)s * ld];
        part = fma(m, sx[c], part);
      }
    }
  }
  spart[q][lane] = part;
  __syncthreads();
  const double res = sb[lane] - ((spart[0][lane] + spart[1][lane]) + (spart[2][lane] + spart[3][lane]));
  __syncthreads();
  if (tid < NB) sx[tid] = res;
  __syncthreads();
  return x + block_gemv(D, trans, sx, spart, lane, q);
}

template <typename T, bool BETA0>
__device__ __forceinline__ void store_res(T *res, int64_t i, double x, double alpha, double beta) {
  res[i] = BETA0 ? (T)(alpha * x) : (T)(alpha * x + beta * (double)res[i]);
}

template <typename T, bool BETA0, bool LDL>
__global__ void __launch_bounds__(kBlock) sweep_kernel(SweepArgs a) {
  __shared__ double sx[NB], sb[NB], spart[4][NB];
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int g = blockIdx.x;
  T *res = (T *)a.res;
  if (g >= a.nchunks) {                                  // epilogue of everything outside the block chunk gd solves
    const int64_t d_lo = a.r0 + (int64_t)a.gd * NB;
    const int64_t dl = a.r1 - d_lo < NB ? a.r1 - d_lo : NB;
    const int64_t idx = (int64_t)(g - a.nchunks) * kBlock + tid;
    if (idx < a.n - dl) {
      const int64_t i = idx < d_lo ? idx : idx + dl;
      store_res<T, BETA0>(res, a.scatter ? a.scatter[i] : i, a.z[i], a.alpha, a.beta);
    }
    return;
  }
  const T *Tm = (const T *)a.Tm;
  const int64_t c_lo = a.r0 + (int64_t)g * NB;
  const int cl = (int)(a.r1 - c_lo < NB ? a.r1 - c_lo : NB);
  if (a.xl > 0) {
    if (tid < NB) sx[tid] = tid < a.xl ? a.z[a.xs + tid] : 0.0;
    __syncthreads();
    if (!a.rowpanel) {
      double acc = 0.0;
      if (lane < cl) {
        const T *row = Tm + (c_lo + lane) + a.xs * a.ld;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const int c = q * 16 + t;
          if (c < a.xl) acc = fma(ld_stream(row + (int64_t)c * a.ld), sx[c], acc);
        }
      }
      spart[q][lane] = acc;
    } else {
      const double xi = sx[lane];
      double val[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int c = q * 16 + t;
        val[t] = (c < cl && lane < a.xl) ? ld_stream(Tm + (a.xs + lane) + (c_lo + c) * a.ld) * xi : 0.0;
      }
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const double s = wave_sum(val[t]);
        if (lane == 0) spart[0][q * 16 + t] = s;
      }
    }
    __syncthreads();
  }
  double b = 0.0;
  if (tid < cl) {
    b = a.v ? (double)((const T *)a.v)[a.gather ? a.gather[c_lo + tid] : c_lo + tid] : a.z[c_lo + tid];
    if constexpr (LDL) {
      if (a.zscale) b *= a.dsc[c_lo + tid];
    }
    if (a.xl > 0) b -= a.rowpanel ? spart[0][tid] : (spart[0][tid] + spart[1][tid]) + (spart[2][tid] + spart[3][tid]);
  }
  if (g != a.gd) {
    if (tid < cl) a.z[c_lo + tid] = b;
    return;
  }
  __syncthreads();                                       // spart is reused below
  if (tid < NB) sb[tid] = b;
  __syncthreads();
  const T *blk = Tm + c_lo + c_lo * a.ld;                // the diagonal block in the triangle
  double x = block_gemv(a.dinv, a.dinv_t != 0, sb, spart, lane, q);
  x = block_refine<T>(blk, a.ld, cl, a.dinv_t != 0, a.tri_upper != 0, a.tri_unit != 0, a.dinv, x, sb, sx, spart, tid, lane, q);
  if (a.dinv2) {
    if constexpr (LDL) {
      if (tid < cl) x *= a.dsc[c_lo + tid];
    }
    if (tid < NB) sb[tid] = x;
    __syncthreads();
    x = block_gemv(a.dinv2, a.dinv2_t != 0, sb, spart, lane, q);
    x = block_refine<T>(blk, a.ld, cl, a.dinv2_t != 0, a.tri2_upper != 0, a.tri2_unit != 0, a.dinv2, x, sb, sx, spart, tid, lane, q);
  }
  if (tid < cl) {
    a.z[c_lo + tid] = x;
    if (a.epi) store_res<T, BETA0>(res, a.scatter ? a.scatter[c_lo + tid] : c_lo + tid, x, a.alpha, a.beta);
  }
}

// ---------------------------------------------------------------------------------------------- block right-hand sides
// The same chain of launches carrying a group of kb <= KB right-hand sides: every element of the panel, of the stored
// inverse and of the diagonal block is loaded ONCE and used for all of them. Per right-hand side the operations and their
// order are those of sweep_kernel (the 16-term fma chains per quarter, (p0 + p1) + (p2 + p3), wave_sum's tree, the
// refinement), so column j of a block apply is the single-vector apply of that column bit for bit. The loops over j are
// unrolled over KB with a wave-uniform guard j < kb, so x[], part[] stay in registers.
constexpr int KB = 8;                // right-hand sides per pass, the grouping of mxlo_gemv_block; 24 KiB of LDS

// block_gemv for kb vectors: x[j] = row `lane` of D sb[j] (D' if trans)
__device__ __forceinline__ void block_gemv_k(const double *__restrict__ D, bool trans, const double (*sb)[NB],
                                             double (*spart)[4][NB], int kb, int lane, int q, double *x) {
  double part[KB];
#pragma unroll
  for (int j = 0; j < KB; ++j) part[j] = 0.0;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int c = q * 16 + t;
    const double d = trans ? D[lane * NB + c] : D[c * NB + lane];
#pragma unroll
    for (int j = 0; j < KB; ++j)
      if (j < kb) part[j] = fma(d, sb[j][c], part[j]);
  }
#pragma unroll
  for (int j = 0; j < KB; ++j)
    if (j < kb) spart[j][q][lane] = part[j];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < KB; ++j)
    if (j < kb) x[j] = (spart[j][0][lane] + spart[j][1][lane]) + (spart[j][2][lane] + spart[j][3][lane]);
  __syncthreads();
}

// block_refine for kb vectors: x[j] += inv(M) (sb[j] - M x[j]); each element of the diagonal block is read once
template <typename T>
__device__ __forceinline__ void block_refine_k(const T *__restrict__ blk, int64_t ld, int cl, bool trans, bool upper, bool unit,
                                               const double *__restrict__ D, double *x, const double (*sb)[NB], double (*sx)[NB],
                                               double (*spart)[4][NB], int kb, int lane, int q) {
#pragma unroll
  for (int j = 0; j < KB; ++j)
    if (j < kb && (j & 3) == q) sx[j][lane] = x[j];      // every wave holds x of all 64 rows: wave q stores columns j = q, q + 4
  __syncthreads();
  double part[KB];
#pragma unroll
  for (int j = 0; j < KB; ++j) part[j] = 0.0;
  if (lane < cl) {
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int c = q * 16 + t;
      if (c < cl) {
        const int r = trans ? c : lane, s = trans ? lane : c;              // M[lane, c] = S[r, s]
        double m = 0.0;
        if (r == s && unit) m = 1.0;
        else if (upper ? r <= s : r >= s) m = (double)blk[r + (int64_t)s * ld];
#pragma unroll
        for (int j = 0; j < KB; ++j)
          if (j < kb) part[j] = fma(m, sx[j][c], part[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < KB; ++j)
    if (j < kb) spart[j][q][lane] = part[j];
  __syncthreads();
  double r[KB];
#pragma unroll
  for (int j = 0; j < KB; ++j)
    if (j < kb) r[j] = sb[j][lane] - ((spart[j][0][lane] + spart[j][1][lane]) + (spart[j][2][lane] + spart[j][3][lane]));
  __syncthreads();
#pragma unroll
  for (int j = 0; j < KB; ++j)
    if (j < kb && (j & 3) == q) sx[j][lane] = r[j];
  __syncthreads();
  double y[KB];
  block_gemv_k(D, trans, sx, spart, kb, lane, q, y);
#pragma unroll
  for (int j = 0; j < KB; ++j)
    if (j < kb) x[j] = x[j] + y[j];
}

// The end of a sweep for entry i of column j, whose solution is x: the alpha/beta epilogue, or (RF, a.xacc) the step of a refined
// apply. RF is a template parameter so that the kernel of the plain block apply stays the code it was.
template <typename T, bool BETA0, bool RF>
__device__ __forceinline__ void finish_entry(const SweepArgs &a, T *res, int64_t o, int64_t i, int j, double x) {
  if constexpr (RF) {
    double *xp = a.xacc + i + (int64_t)j * a.n;
    if (a.xmode == 1) { *xp = x; return; }
    x = *xp + x;
    if (a.xmode == 2) { *xp = x; return; }
  }
  store_res<T, BETA0>(res + (int64_t)j * a.ldr, o, x, a.alpha, a.beta);
}

template <typename T, bool BETA0, bool LDL, bool RF>
__global__ void __launch_bounds__(kBlock) sweep_block_kernel(SweepArgs a) {
  __shared__ double sx[KB][NB], sb[KB][NB], spart[KB][4][NB];
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int g = blockIdx.x, kb = a.kb;
  T *res = (T *)a.res;
  if (g >= a.nchunks) {                                  // epilogue of everything outside the block chunk gd solves
    const int64_t d_lo = a.r0 + (int64_t)a.gd * NB;
    const int64_t dl = a.r1 - d_lo < NB ? a.r1 - d_lo : NB;
    const int64_t idx = (int64_t)(g - a.nchunks) * kBlock + tid;
    if (idx < a.n - dl) {
      const int64_t i = idx < d_lo ? idx : idx + dl;
      const int64_t o = a.scatter ? a.scatter[i] : i;
#pragma unroll
      for (int j = 0; j < KB; ++j)
        if (j < kb) finish_entry<T, BETA0, RF>(a, res, o, i, j, a.z[i + (int64_t)j * a.n]);
    }
    return;
  }
  const T *Tm = (const T *)a.Tm;
  const int64_t c_lo = a.r0 + (int64_t)g * NB;
  const int cl = (int)(a.r1 - c_lo < NB ? a.r1 - c_lo : NB);
  if (a.xl > 0) {
    for (int e = tid; e < kb * NB; e += kBlock) {
      const int j = e >> 6, r = e & 63;
      sx[j][r] = r < a.xl ? a.z[a.xs + r + (int64_t)j * a.n] : 0.0;
    }
    __syncthreads();
    if (!a.rowpanel) {                                   // the thread's panel element stays in a register for the kb columns
      double acc[KB];
#pragma unroll
      for (int j = 0; j < KB; ++j) acc[j] = 0.0;
      if (lane < cl) {
        const T *row = Tm + (c_lo + lane) + a.xs * a.ld;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const int c = q * 16 + t;
          if (c < a.xl) {
            const double tv = ld_stream(row + (int64_t)c * a.ld);
#pragma unroll
            for (int j = 0; j < KB; ++j)
              if (j < kb) acc[j] = fma(tv, sx[j][c], acc[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < KB; ++j)
        if (j < kb) spart[j][q][lane] = acc[j];
    } else {                                             // the 16 loaded elements are kept; one wave_sum per (panel column, rhs)
      double tv[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int c = q * 16 + t;
        tv[t] = (c < cl && lane < a.xl) ? ld_stream(Tm + (a.xs + lane) + (c_lo + c) * a.ld) : 0.0;
      }
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        if (j < kb) {
          const double xi = sx[j][lane];
#pragma unroll
          for (int t = 0; t < 16; ++t) {
            const int c = q * 16 + t;
            const double s = wave_sum((c < cl && lane < a.xl) ? tv[t] * xi : 0.0);
            if (lane == 0) spart[j][0][c] = s;
          }
        }
      }
    }
    __syncthreads();
  }
  double b[KB];
#pragma unroll
  for (int j = 0; j < KB; ++j) b[j] = 0.0;
  if (tid < cl) {
    const int64_t i = c_lo + tid;
    const int64_t src = (a.v && a.gather) ? a.gather[i] : i;     // perm[i] is read once per row
    double dsc = 1.0;
    if constexpr (LDL) {
      if (a.zscale) dsc = a.dsc[i];
    }
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      if (j < kb) {
        double bj = a.v ? (double)((const T *)a.v)[src + (int64_t)j * a.ldv] : a.z[i + (int64_t)j * a.n];
        if constexpr (LDL) {
          if (a.zscale) bj *= dsc;
        }
        if (a.xl > 0)
          bj -= a.rowpanel ? spart[j][0][tid] : (spart[j][0][tid] + spart[j][1][tid]) + (spart[j][2][tid] + spart[j][3][tid]);
        b[j] = bj;
      }
    }
  }
  if (g != a.gd) {
    if (tid < cl) {
#pragma unroll
      for (int j = 0; j < KB; ++j)
        if (j < kb) a.z[c_lo + tid + (int64_t)j * a.n] = b[j];
    }
    return;
  }
  __syncthreads();                                       // spart is reused below
  if (tid < NB) {
#pragma unroll
    for (int j = 0; j < KB; ++j)
      if (j < kb) sb[j][tid] = b[j];
  }
  __syncthreads();
  const T *blk = Tm + c_lo + c_lo * a.ld;                // the diagonal block in the triangle
  double x[KB];
  block_gemv_k(a.dinv, a.dinv_t != 0, sb, spart, kb, lane, q, x);
  block_refine_k<T>(blk, a.ld, cl, a.dinv_t != 0, a.tri_upper != 0, a.tri_unit != 0, a.dinv, x, sb, sx, spart, kb, lane, q);
  if (a.dinv2) {
    if constexpr (LDL) {
      if (lane < cl) {
        const double dsc = a.dsc[c_lo + lane];
#pragma unroll
        for (int j = 0; j < KB; ++j)
          if (j < kb) x[j] *= dsc;
      }
    }
#pragma unroll
    for (int j = 0; j < KB; ++j)
      if (j < kb && (j & 3) == q) sb[j][lane] = x[j];
    __syncthreads();
    block_gemv_k(a.dinv2, a.dinv2_t != 0, sb, spart, kb, lane, q, x);
    block_refine_k<T>(blk, a.ld, cl, a.dinv2_t != 0, a.tri2_upper != 0, a.tri2_unit != 0, a.dinv2, x, sb, sx, spart, kb, lane, q);
  }
  if (tid < cl) {
    const int64_t i = c_lo + tid;
    const int64_t o = (a.epi && a.scatter) ? a.scatter[i] : i;
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      if (j < kb) {
        a.z[i + (int64_t)j * a.n] = x[j];
        if (a.epi) finish_entry<T, BETA0, RF>(a, res, o, i, j, x[j]);
      }
    }
  }
}

template <typename T, bool LDL>
int32_t launch_sweep_as(mxlo_ctx *ctx, const SweepArgs &a) {
  int64_t grid = a.nchunks;
  if (a.epi) {
    const int64_t d_lo = a.r0 + (int64_t)a.gd * NB, dl = a.r1 - d_lo < NB ? a.r1 - d_lo : NB;
    grid += (a.n - dl + kBlock - 1) / kBlock;
  }
  MXLO_REQUIRE(grid < (1LL << 31), MXLO_ESHAPE, "triangular solve: n = %lld is too large", (long long)a.n);
  if (a.kb > 0 && a.xacc) {                              // a refined apply: the block kernel with the iterate's epilogue
    if (a.beta == 0.0) hipLaunchKernelGGL((sweep_block_kernel<T, true, LDL, true>), dim3((unsigned)grid), dim3(kBlock), 0, ctx->stream, a);
    else hipLaunchKernelGGL((sweep_block_kernel<T, false, LDL, true>), dim3((unsigned)grid), dim3(kBlock), 0, ctx->stream, a);
  } else if (a.kb > 0) {                                 // a group of right-hand sides: the same grid, the block kernel
    if (a.beta == 0.0) hipLaunchKernelGGL((sweep_block_kernel<T, true, LDL, false>), dim3((unsigned)grid), dim3(kBlock), 0, ctx->stream, a);
    else hipLaunchKernelGGL((sweep_block_kernel<T, false, LDL, false>), dim3((unsigned)grid), dim3(kBlock), 0, ctx->stream, a);
  } else if (a.beta == 0.0) hipLaunchKernelGGL((sweep_kernel<T, true, LDL>), dim3((unsigned)grid), dim3(kBlock), 0, ctx->stream, a);
  else hipLaunchKernelGGL((sweep_kernel<T, false, LDL>), dim3((unsigned)grid), dim3(kBlock), 0, ctx->stream, a);
  MXLO_LAUNCH_CHECK();
  return MXLO_OK;
}

// the kernels of opLDL are those of a launch that carries the pivots
template <typename T>
int32_t launch_sweep(mxlo_ctx *ctx, const SweepArgs &a) {
  return a.dsc ? launch_sweep_as<T, true>(ctx, a) : launch_sweep_as<T, false>(ctx, a);
}

// A sweep is described by three structs, written at the call as designated initialisers that name what is not the default.

// the columns of a block apply that one chain of launches takes; kb == 0: a vector apply, on the vector kernels
struct Group {
  int kb = 0;                          // kb > 0: v and res are n x kb (ldv, ldr), z is n x kb with column stride n; the same launches
  int64_t ldr = 0, ldv = 0;
};

// what the sweeps and the reflector chains of one apply, or of one group of its columns, share
template <typename T>
struct Apply {
  mxlo_ctx *ctx;
  T *res;                              // written by the launch with the epilogue only: res = alpha x + beta res
  double alpha, beta;
  double *z;                           // the work matrix: the right-hand side turning into the solution
  Group grp = {};
  double *xacc = nullptr;              // a refined apply (block form only): the iterate; the launch with the epilogue then ends as
  int xmode = 0;                       // xmode says (SweepArgs) instead of writing res
};

// the triangle of a sweep and the inverses of its diagonal blocks
template <typename T>
struct Tri {
  const T *Tm;
  int64_t ld, n;
  bool upper = false;
  // opLU, pivoted opLDL: a lower triangle is L, with an implicit unit diagonal, and the turn-around block (Sweep::tdinv) is the
  // OTHER triangle of the same storage
  bool unit_lower = false;
  const double *dinv;                  // the stored inverses of the NB x NB diagonal blocks, one per block column
};

// One sweep: solves op(T) x = rhs. `ascending` = (lower, N) or (upper, T); the panel of a transposed solve is a block ROW.
template <typename T>
struct Sweep {
  bool trans = false;
  const T *v = nullptr;                // the right-hand side of a first sweep; NULL (a refined apply): z already holds it, the residual
  bool first = true;                   // the right-hand side comes from v; else z holds it and its first block is already solved
  bool turn = false;                   // after the last block, multiply it by its transposed inverse once more (the first block of
                                       // the Cholesky back sweep)
  bool epi = false;                    // fuse the alpha/beta epilogue into the last launch
  const double *dsc = nullptr;         // opLDL: the pivots; they multiply the turn-around block between its two products and, in a
                                       // sweep that continues (!first), every other block as the first launch reads it
  const double *tdinv = nullptr;       // opLU: the turn-around multiplies by the last block of THESE inverses, transposed like the
                                       // sweep itself, instead
  const int *gather = nullptr;         // the permutation the first launch reads v through ...
  const int *scatter = nullptr;        // ... and the one the epilogue writes res through
};

template <typename T>
int32_t sweep(const Apply<T> &ap, const Tri<T> &t, const Sweep<T> &s) {
  const int64_t n = t.n, nb = (n + NB - 1) / NB;
  const bool asc = t.upper == s.trans;
  SweepArgs a{};
  a.Tm = t.Tm; a.ld = t.ld; a.n = n; a.z = ap.z; a.rowpanel = s.trans; a.dinv_t = s.trans; a.res = ap.res; a.alpha = ap.alpha;
  a.beta = ap.beta; a.dsc = s.dsc; a.gather = s.gather; a.scatter = s.scatter; a.dinv2_t = s.tdinv ? s.trans : 1;
  a.kb = ap.grp.kb; a.ldr = ap.grp.ldr; a.ldv = ap.grp.ldv; a.xacc = ap.xacc; a.xmode = ap.xmode;
  const bool upper2 = s.tdinv ? !t.upper : t.upper;
  a.tri_upper = t.upper; a.tri_unit = t.unit_lower && !t.upper; a.tri2_upper = upper2; a.tri2_unit = t.unit_lower && !upper2;
  const int64_t kfirst = asc ? 0 : nb - 1, klast = asc ? nb - 1 : 0, step = asc ? 1 : -1;
  const double *tblock = (s.tdinv ? s.tdinv : t.dinv) + klast * NB2;
  if (s.first) {                                          // z = v, and the first block solved
    a.v = s.v; a.xl = 0; a.r0 = 0; a.r1 = n; a.nchunks = (int)nb; a.gd = (int)kfirst;
    a.dinv = t.dinv + kfirst * NB2;
    a.dinv2 = (s.turn && nb == 1) ? tblock : nullptr;
    a.epi = s.epi && nb == 1;
    MXLO_TRY(launch_sweep<T>(ap.ctx, a));
    a.v = nullptr;
  }
  for (int64_t k = kfirst; k != klast; k += step) {       // panel k, then block k + step
    const int64_t kn = k + step;
    a.xs = k * NB;
    a.xl = (int)(n - a.xs < NB ? n - a.xs : NB);
    if (asc) { a.r0 = (k + 1) * NB; a.r1 = n; a.gd = 0; }
    else { a.r0 = 0; a.r1 = k * NB; a.gd = (int)(k - 1); }
    a.nchunks = (int)((a.r1 - a.r0 + NB - 1) / NB);
    a.dinv = t.dinv + kn * NB2;
    a.dinv2 = (s.turn && kn == klast) ? tblock : nullptr;
    a.epi = s.epi && kn == klast;
    a.zscale = s.dsc && !s.first && k == kfirst;
    MXLO_TRY(launch_sweep<T>(ap.ctx, a));
  }
  return MXLO_OK;
}

// ---------------------------------------------------------------------------------------------- the host checks
// Every entry point below refuses a bad call before anything is launched, through the functions of this section. What an
// operator adds is a LIST of the buffers it owns ({pointer, bytes, name}), never a check of its own: disjoint() holds a
// factorisation's buffers against each other, check_operands() res and V of an apply against the operator's.
struct Buf {
  const void *p;
  int64_t bytes;
  const char *name;
};

inline int64_t esize(int32_t dtype) { return dtype == MXLO_F64 ? 8 : 4; }
inline int64_t mat_bytes(int64_t rows, int64_t cols, int64_t ld, int64_t es) { return ((cols - 1) * ld + rows) * es; }
inline int64_t blocks_bytes(int64_t n) { return (n + NB - 1) / NB * NB2 * 8; }   // one NB x NB block of doubles per block column

// calls f.template operator()<T>() for the element type of dtype, which the entry point has checked
template <typename F>
int32_t with_real(int32_t dtype, F &&f) {
  return dtype == MXLO_F64 ? f.template operator()<double>() : f.template operator()<float>();
}

int32_t check_real(mxlo_ctx *ctx, int32_t dtype, const char *what) {
  MXLO_REQUIRE(ctx, MXLO_EINVAL, "%s: null ctx", what);
  MXLO_REQUIRE(dtype == MXLO_F64 || dtype == MXLO_F32, MXLO_EINVAL, "%s: real Float64 / Float32 only", what);
  return MXLO_OK;
}

int32_t check_mode(int32_t op_mode, const char *what) {
  MXLO_REQUIRE(op_mode == MXLO_OP_N || op_mode == MXLO_OP_T || op_mode == MXLO_OP_C, MXLO_EINVAL, "%s: op_mode %d", what, op_mode);
  return MXLO_OK;
}

int32_t check_common(mxlo_ctx *ctx, int32_t dtype, const void *A, int64_t ld, int64_t n, const char *what) {
  MXLO_TRY(check_real(ctx, dtype, what));
  MXLO_REQUIRE(n >= 0 && ld >= (n > 1 ? n : 1), MXLO_ESHAPE, "%s: n = %lld, ld = %lld", what, (long long)n, (long long)ld);
  MXLO_REQUIRE(A || n == 0, MXLO_EINVAL, "%s: null matrix", what);
  return MXLO_OK;
}

// the buffers of a factorisation may not overlap each other; an operand that may be NULL (M) is skipped when it is
int32_t disjoint(std::initializer_list<Buf> bufs, const char *what) {
  for (const Buf *x = bufs.begin(); x != bufs.end(); ++x)
    for (const Buf *y = x + 1; y != bufs.end(); ++y)
      MXLO_REQUIRE(!x->p || !y->p || !bytes_overlap(x->p, x->bytes, y->p, y->bytes), MXLO_EINVAL, "%s: %s overlaps %s", what, x->name,
                   y->name);
  return MXLO_OK;
}

// x against each of `others`, which may overlap one another (operands that are only read)
int32_t apart(const Buf &x, std::initializer_list<Buf> others, const char *what) {
  for (const Buf &y : others) MXLO_TRY(disjoint({x, y}, what));
  return MXLO_OK;
}

// the tail of a factorisation: it reads `count` info words back, the only synchronisation, which a graph capture cannot hold.
// refuse_capture() is the last check before the device is touched, read_back() the last call of the chain.
int32_t refuse_capture(const mxlo_ctx *ctx, const char *what) {
  MXLO_REQUIRE(!ctx->capturing, MXLO_ESTATE, "%s: reads its info words back, which a graph capture cannot hold", what);
  return MXLO_OK;
}

int32_t read_back(mxlo_ctx *ctx, const int32_t *info_dev, int32_t *words, int count) {
  MXLO_HIP(hipMemcpyAsync(words, info_dev, count * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  MXLO_HIP(hipStreamSynchronize(ctx->stream));
  return MXLO_OK;
}

// res (rrows x k, ldr) and V (vrows x k, ldv) of an apply, columns of unit stride. A vector entry point passes vectors():
// one column in a leading dimension of max(1, rows); a _block entry point passes columns(), and takes the block kernels
// whatever k is.
struct Operands {
  const void *res, *v;
  int64_t k, ldr, ldv, rrows, vrows;
  bool block;
};
inline Operands vectors(const void *res, const void *v, int64_t rrows, int64_t vrows) {
  return {res, v, 1, rrows > 1 ? rrows : 1, vrows > 1 ? vrows : 1, rrows, vrows, false};
}
inline Operands columns(const void *res, int64_t ldr, const void *v, int64_t ldv, int64_t k, int64_t rrows, int64_t vrows) {
  return {res, v, k, ldr, ldv, rrows, vrows, true};
}

// res and V against the buffers an operator owns, none of which may be NULL
int32_t check_owned(int32_t dtype, const Operands &o, std::initializer_list<Buf> own, const char *what) {
  const int64_t es = esize(dtype), rb = mat_bytes(o.rrows, o.k, o.ldr, es), vb = mat_bytes(o.vrows, o.k, o.ldv, es);
  for (const Buf &b : own) {
    MXLO_REQUIRE(b.p, MXLO_EINVAL, "%s: null operand (%s)", what, b.name);
    MXLO_REQUIRE(!bytes_overlap(o.res, rb, b.p, b.bytes) && !bytes_overlap(o.v, vb, b.p, b.bytes), MXLO_EINVAL,
                 "%s: res or V overlaps %s", what, b.name);
  }
  return MXLO_OK;
}

// The checks every apply shares once its operator's shape is known to be valid: k and the leading dimensions, the null
// operands, the rule for res and V, and both against `own`. go: whether there is anything to do — with k == 0, or `empty`
// (n == 0), the call is MXLO_OK and launches nothing, and what comes after the leading dimensions is not looked at. Every
// entry point runs the checks it has of its own and then returns on !go. res may be V only as the same matrix: the same
// pointer, the same leading dimension and the same number of rows, which for a rectangular operator means mf == nf.
int32_t check_operands(int32_t dtype, const Operands &o, bool empty, std::initializer_list<Buf> own, const char *what, bool &go) {
  go = false;
  MXLO_REQUIRE(o.k >= 0 && o.ldr >= (o.rrows > 1 ? o.rrows : 1) && o.ldv >= (o.vrows > 1 ? o.vrows : 1), MXLO_ESHAPE,
               "%s: k = %lld, ldr = %lld for %lld rows, ldv = %lld for %lld rows", what, (long long)o.k, (long long)o.ldr,
               (long long)o.rrows, (long long)o.ldv, (long long)o.vrows);
  if (empty || o.k == 0) return MXLO_OK;
  MXLO_REQUIRE(o.res && o.v, MXLO_EINVAL, "%s: null operand (res / V)", what);
  const int64_t es = esize(dtype);
  MXLO_REQUIRE((o.res == o.v && o.ldr == o.ldv && o.rrows == o.vrows) ||
                   !bytes_overlap(o.res, mat_bytes(o.rrows, o.k, o.ldr, es), o.v, mat_bytes(o.vrows, o.k, o.ldv, es)),
               MXLO_EINVAL, "%s: res overlaps V without being V (only mul!(X, op, X) of a square operator, as the same matrix, is defined)",
               what);
  MXLO_TRY(check_owned(dtype, o, own, what));
  go = true;
  return MXLO_OK;
}

// a square apply: A (n x n, ld), its block inverses, work of n * min(k, KB) doubles, and what the operator owns besides
int32_t check_apply(mxlo_ctx *ctx, int32_t dtype, const Operands &o, const void *A, int64_t ld, int64_t n, const double *dinv,
                    const double *work, const char *what, bool &go, std::initializer_list<Buf> more = {}) {
  go = false;
  MXLO_TRY(check_common(ctx, dtype, A, ld, n, what));
  MXLO_TRY(check_operands(dtype, o, n == 0,
                          {{A, mat_bytes(n, n, ld, esize(dtype)), "the matrix"},
                           {dinv, blocks_bytes(n), "the block inverses"},
                           {work, n * (o.k < KB ? o.k : KB) * 8, "the work vector"}},
                          what, go));
  return go ? check_owned(dtype, o, more, what) : MXLO_OK;
}

// opLU's applies: the second set of block inverses and the permutation besides
int32_t check_lu_apply(mxlo_ctx *ctx, int32_t dtype, const Operands &o, const void *W, int64_t ld, int64_t n, const double *dinv_l,
                       const double *dinv_u, const int32_t *perm, const double *work, const char *what, bool &go) {
  return check_apply(ctx, dtype, o, W, ld, n, dinv_l, work, what, go,
                     {{dinv_u, blocks_bytes(n), "the block inverses of U"}, {perm, n * 4, "the permutation"}});
}

template <typename T>
int32_t getrf_t(mxlo_ctx *ctx, const T *M, int64_t ldm, T *W, int64_t ldw, int64_t n, double *dinv_l, double *dinv_u, int *perm,
                int *info_dev) {
  const int64_t nb = (n + NB - 1) / NB;
  MXLO_HIP(hipMemsetAsync(info_dev, 0, sizeof(int), ctx->stream));
  hipLaunchKernelGGL((getrf_copy_kernel<T>), dim3((unsigned)((n + kBlock - 1) / kBlock), (unsigned)(n < 1024 ? n : 1024)), dim3(kBlock),
                     0, ctx->stream, W, ldw, M, ldm, n, perm);
  MXLO_LAUNCH_CHECK();
  for (int64_t k = 0; k < nb; ++k) {
    const int64_t j0 = k * NB, jb = n - j0 < NB ? n - j0 : NB, j1 = j0 + jb, m = n - j1;
    hipLaunchKernelGGL((getrf_panel_kernel<T>), dim3(1), dim3(PT), 0, ctx->stream, W, ldw, n, j0, (int)jb, perm, info_dev);
    MXLO_LAUNCH_CHECK();
    hipLaunchKernelGGL((getrf_inv_kernel<T>), dim3(2), dim3(kBlock), 0, ctx->stream, (const T *)W, ldw, n, j0, dinv_l + k * NB2,
                       dinv_u + k * NB2, (const int *)info_dev);
    MXLO_LAUNCH_CHECK();
    if (n > jb) {
      hipLaunchKernelGGL((getrf_swap_kernel<T>), dim3((unsigned)((n - jb + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, W, ldw,
                         n, j0, (int)jb, (const int *)perm, (const int *)info_dev);
      MXLO_LAUNCH_CHECK();
    }
    if (m <= 0) break;
    const unsigned tiles = (unsigned)((m + NB - 1) / NB);
    hipLaunchKernelGGL((getrf_row_kernel<T>), dim3(tiles), dim3(kBlock), 0, ctx->stream, W, ldw, n, j0, (int)jb,
                       (const double *)(dinv_l + k * NB2), (const int *)info_dev);
    MXLO_LAUNCH_CHECK();
    hipLaunchKernelGGL((getrf_gemm_kernel<T>), dim3(tiles, tiles), dim3(kBlock), 0, ctx->stream, W + j1 + j1 * ldw,
                       (const T *)(W + j1 + j0 * ldw), (const T *)(W + j0 + j1 * ldw), ldw, (int)m, (int)jb, (const int *)info_dev);
    MXLO_LAUNCH_CHECK();
  }
  return MXLO_OK;
}

// A = P' L U. N: x = inv(U) inv(L) (P v) — v gathered, the unit lower sweep, the upper one. T: A' = U' L' P, x = P' inv(L') inv(U') v —
// the U' sweep, the L' sweep, the epilogue scattered.
template <typename T>
int32_t lu_mul_t(const Apply<T> &ap, const T *W, int64_t ld, int64_t n, const double *dinv_l, const double *dinv_u, const int *perm,
                 const T *v, bool trans) {
  const bool one = n <= NB;
  const double *d1 = trans ? dinv_u : dinv_l, *d2 = trans ? dinv_l : dinv_u;
  const int *gather = (trans || !v) ? nullptr : perm, *scatter = trans ? perm : nullptr;   // a residual (!v) is already in the sweep's order
  MXLO_TRY(sweep(ap, {.Tm = W, .ld = ld, .n = n, .upper = trans, .unit_lower = true, .dinv = d1},
                 {.trans = trans, .v = v, .turn = true, .epi = one, .tdinv = d2, .gather = gather, .scatter = scatter}));
  if (one) return MXLO_OK;
  return sweep(ap, {.Tm = W, .ld = ld, .n = n, .upper = !trans, .unit_lower = true, .dinv = d2},
               {.trans = trans, .first = false, .epi = true, .scatter = scatter});
}

// x = L^{-T} (L^{-1} v), or with the pivots d (opLDL, Lt = L D) x = Lt^{-T} (d .* (Lt^{-1} v)): the same two sweeps; where the
// pivots come in is said at Sweep::dsc
template <typename T>
int32_t sym_mul_t(const Apply<T> &ap, const T *L, int64_t ld, int64_t n, const double *dinv, const double *d, const T *v) {
  const bool one = n <= NB;                              // a single block: both products and the epilogue in one launch
  const Tri<T> t{.Tm = L, .ld = ld, .n = n, .dinv = dinv};
  MXLO_TRY(sweep(ap, t, {.v = v, .turn = true, .epi = one, .dsc = d}));
  if (one) return MXLO_OK;
  return sweep(ap, t, {.trans = true, .first = false, .epi = true, .dsc = d});
}

// LDL: the chain of mxlo_ldlt — the same launches with the LDL' diagonal step and the pivots d handed to phases (b) and (c)
template <typename T, bool LDL>
int32_t potrf_t(mxlo_ctx *ctx, const T *M, int64_t ldm, int rowmajor, T *W, int64_t ldw, int64_t n, double *dinv, double *d,
                int *info_dev) {
  const int64_t nb = (n + NB - 1) / NB;
  MXLO_HIP(hipMemsetAsync(info_dev, 0, sizeof(int), ctx->stream));
  if (M) {
    hipLaunchKernelGGL((pack_upper_kernel<T>), dim3((unsigned)nb, (unsigned)nb), dim3(kBlock), 0, ctx->stream, W, ldw, M, ldm,
                       rowmajor, n);
    MXLO_LAUNCH_CHECK();
  }
  for (int64_t k = 0; k < nb; ++k) {
    const int64_t j0 = k * NB, jb = n - j0 < NB ? n - j0 : NB, j1 = j0 + jb, m = n - j1;
    if constexpr (LDL) hipLaunchKernelGGL((ldlt_diag_kernel<T>), dim3(1), dim3(kBlock), 0, ctx->stream, W, ldw, n, j0, dinv + k * NB2, d, info_dev);
    else hipLaunchKernelGGL((potrf_diag_kernel<T>), dim3(1), dim3(kBlock), 0, ctx->stream, W, ldw, n, j0, dinv + k * NB2, info_dev);
    MXLO_LAUNCH_CHECK();
    if (m <= 0) break;
    const unsigned tiles = (unsigned)((m + NB - 1) / NB);
    hipLaunchKernelGGL((potrf_panel_kernel<T, LDL>), dim3(tiles), dim3(kBlock), 0, ctx->stream, W, ldw, n, j0, (int)jb,
                       (const double *)(dinv + k * NB2), (const double *)d, (const int *)info_dev);
    MXLO_LAUNCH_CHECK();
    hipLaunchKernelGGL((potrf_syrk_kernel<T, LDL>), dim3(tiles, tiles), dim3(kBlock), 0, ctx->stream, W + j1 + j1 * ldw,
                       (const T *)(W + j1 + j0 * ldw), ldw, (int)m, (int)jb, (const double *)(LDL ? d + j0 : nullptr),
                       (const int *)info_dev);
    MXLO_LAUNCH_CHECK();
  }
  return MXLO_OK;
}

}  // namespace

MXLO_API int32_t mxlo_tri_kind(mxlo_ctx *ctx, int32_t dtype, const void *M, int64_t ld, int64_t n, int32_t *kind_dev) {
  MXLO_TRY(check_common(ctx, dtype, M, ld, n, "mxlo_tri_kind"));
  MXLO_REQUIRE(kind_dev, MXLO_EINVAL, "mxlo_tri_kind: null result word");
  MXLO_DEVICE_GUARD(ctx);
  MXLO_HIP(hipMemsetAsync(kind_dev, 0, sizeof(int32_t), ctx->stream));
  if (n == 0) return MXLO_OK;
  const unsigned grid = (unsigned)(n < 4096 ? n : 4096);
  if (dtype == MXLO_F64) hipLaunchKernelGGL((tri_kind_kernel<double>), dim3(grid), dim3(kBlock), 0, ctx->stream, (const double *)M, ld, n, kind_dev);
  else hipLaunchKernelGGL((tri_kind_kernel<float>), dim3(grid), dim3(kBlock), 0, ctx->stream, (const float *)M, ld, n, kind_dev);
  MXLO_LAUNCH_CHECK();
  return MXLO_OK;
}

MXLO_API int32_t mxlo_tri_prepare(mxlo_ctx *ctx, int32_t dtype, const void *Tm, int64_t ld, int64_t n, int32_t upper, double *dinv) {
  MXLO_TRY(check_common(ctx, dtype, Tm, ld, n, "mxlo_tri_prepare"));
  if (n == 0) return MXLO_OK;
  MXLO_REQUIRE(dinv, MXLO_EINVAL, "mxlo_tri_prepare: null storage for the block inverses");
  MXLO_DEVICE_GUARD(ctx);
  const unsigned nb = (unsigned)((n + NB - 1) / NB);
  if (dtype == MXLO_F64) hipLaunchKernelGGL((tri_prepare_kernel<double>), dim3(nb), dim3(kBlock), 0, ctx->stream, (const double *)Tm, ld, n, upper ? 1 : 0, dinv);
  else hipLaunchKernelGGL((tri_prepare_kernel<float>), dim3(nb), dim3(kBlock), 0, ctx->stream, (const float *)Tm, ld, n, upper ? 1 : 0, dinv);
  MXLO_LAUNCH_CHECK();
  return MXLO_OK;
}

namespace {
// mxlo_potrf (d == NULL) and mxlo_ldlt: the checks, the chain of launches, the one copy of the info word
int32_t factor(mxlo_ctx *ctx, int32_t dtype, const void *M, int64_t ldm, int32_t m_rowmajor, void *W, int64_t ldw, int64_t n,
               double *dinv, double *d, int32_t *info_dev, int32_t *info, const char *what) {
  MXLO_TRY(check_common(ctx, dtype, W, ldw, n, what));
  MXLO_REQUIRE(info, MXLO_EINVAL, "%s: null info", what);
  *info = 0;
  if (n == 0) return MXLO_OK;
  MXLO_REQUIRE(dinv && info_dev, MXLO_EINVAL, "%s: null storage for the block inverses / the info word", what);
  MXLO_REQUIRE(n < (1LL << 31) - NB, MXLO_ESHAPE, "%s: n = %lld is too large", what, (long long)n);
  if (M) MXLO_REQUIRE(ldm >= (n > 1 ? n : 1), MXLO_ESHAPE, "%s: ldm = %lld < n", what, (long long)ldm);
  const int64_t es = esize(dtype);
  const Buf w{W, mat_bytes(n, n, ldw, es), "the factor"};   // the block inverses are held against the pivots only
  MXLO_TRY(disjoint({{M, M ? mat_bytes(n, n, ldm, es) : 0, "M"}, w}, what));
  MXLO_TRY(apart({d, n * 8, "the pivots' storage"}, {w, {dinv, blocks_bytes(n), "the block inverses"}}, what));
  MXLO_TRY(refuse_capture(ctx, what));
  MXLO_DEVICE_GUARD(ctx);
  MXLO_TRY(with_real(dtype, [&]<typename T>() {
    if (d) return potrf_t<T, true>(ctx, (const T *)M, ldm, m_rowmajor, (T *)W, ldw, n, dinv, d, info_dev);
    return potrf_t<T, false>(ctx, (const T *)M, ldm, m_rowmajor, (T *)W, ldw, n, dinv, d, info_dev);
  }));
  return read_back(ctx, info_dev, info, 1);
}
}  // namespace

MXLO_API int32_t mxlo_potrf(mxlo_ctx *ctx, int32_t dtype, const void *M, int64_t ldm, int32_t m_rowmajor, void *W, int64_t ldw,
                            int64_t n, double *dinv, int32_t *info_dev, int32_t *info) {
  return factor(ctx, dtype, M, ldm, m_rowmajor, W, ldw, n, dinv, nullptr, info_dev, info, "mxlo_potrf");
}

MXLO_API int32_t mxlo_ldlt(mxlo_ctx *ctx, int32_t dtype, const void *M, int64_t ldm, int32_t m_rowmajor, void *W, int64_t ldw,
                           int64_t n, double *dinv, double *d, int32_t *info_dev, int32_t *info) {
  MXLO_REQUIRE(d || n == 0, MXLO_EINVAL, "mxlo_ldlt: null storage for the pivots");
  return factor(ctx, dtype, M, ldm, m_rowmajor, W, ldw, n, dinv, d, info_dev, info, "mxlo_ldlt");
}

// ---------------------------------------------------------------------------------------------- the applies' entry points
// A vector entry point and its _block form share one body, which takes the Operands. The n x k operands of the block form
// go through the chain in groups of KB columns: one chain of launches and one read of the factor per group. A group's
// columns of V are read completely by its first launch and its columns of res written only by its last, and the groups are
// different columns, so res may be V (the same pointer and leading dimension).
namespace {
template <typename T, typename F>
int32_t for_groups(T *res, int64_t ldr, const T *V, int64_t ldv, int64_t k, F &&apply) {
  for (int64_t j0 = 0; j0 < k; j0 += KB) {
    Group grp;
    grp.kb = (int)(k - j0 < KB ? k - j0 : KB);
    grp.ldr = ldr;
    grp.ldv = ldv;
    MXLO_TRY(apply(res + j0 * ldr, V + j0 * ldv, grp));
  }
  return MXLO_OK;
}

// The one fork between the two forms: f(res_j, V_j, grp), a generic lambda over the element type, is called once with
// Group{} for a vector entry point, which so keeps the vector kernels, and per group of KB columns for a block one
template <typename F>
int32_t for_real_groups(int32_t dtype, const Operands &o, F &&f) {
  return with_real(dtype, [&]<typename T>() {
    if (!o.block) return f((T *)o.res, (const T *)o.v, Group{});
    return for_groups((T *)o.res, o.ldr, (const T *)o.v, o.ldv, o.k, f);
  });
}

int32_t trisolve_mul(mxlo_ctx *ctx, int32_t dtype, const Operands &o, const void *Tm, int64_t ld, int64_t n, int32_t upper,
                     int32_t op_mode, const double *dinv, double *work, double alpha, double beta, const char *what) {
  bool go;
  MXLO_TRY(check_apply(ctx, dtype, o, Tm, ld, n, dinv, work, what, go));
  MXLO_TRY(check_mode(op_mode, what));
  if (!go) return MXLO_OK;
  MXLO_DEVICE_GUARD(ctx);
  const bool tr = op_mode != MXLO_OP_N, up = upper != 0;
  return for_real_groups(dtype, o, [&]<typename T>(T *r, const T *v, Group grp) {
    return sweep<T>({ctx, r, alpha, beta, work, grp}, {.Tm = (const T *)Tm, .ld = ld, .n = n, .upper = up, .dinv = dinv},
                    {.trans = tr, .v = v, .epi = true});
  });
}

// mxlo_chol_mul* and, with the pivots d, mxlo_ldl_mul*
int32_t sym_mul(mxlo_ctx *ctx, int32_t dtype, const Operands &o, const void *L, int64_t ld, int64_t n, const double *dinv,
                const double *d, bool ldl, double *work, double alpha, double beta, const char *what) {
  bool go;
  MXLO_TRY(check_apply(ctx, dtype, o, L, ld, n, dinv, work, what, go));
  if (ldl && go) MXLO_TRY(check_owned(dtype, o, {{d, n * 8, "the pivots"}}, what));
  if (!go) return MXLO_OK;
  MXLO_DEVICE_GUARD(ctx);
  return for_real_groups(dtype, o, [&]<typename T>(T *r, const T *v, Group grp) {
    return sym_mul_t<T>({ctx, r, alpha, beta, work, grp}, (const T *)L, ld, n, dinv, d, v);
  });
}

int32_t lu_mul(mxlo_ctx *ctx, int32_t dtype, const Operands &o, const void *W, int64_t ldw, int64_t n, const double *dinv_l,
               const double *dinv_u, const int32_t *perm, double *work, int32_t op_mode, double alpha, double beta, const char *what) {
  bool go;
  MXLO_TRY(check_lu_apply(ctx, dtype, o, W, ldw, n, dinv_l, dinv_u, perm, work, what, go));
  MXLO_TRY(check_mode(op_mode, what));
  if (!go) return MXLO_OK;
  MXLO_DEVICE_GUARD(ctx);
  const bool tr = op_mode != MXLO_OP_N;
  return for_real_groups(dtype, o, [&]<typename T>(T *r, const T *v, Group grp) {
    return lu_mul_t<T>({ctx, r, alpha, beta, work, grp}, (const T *)W, ldw, n, dinv_l, dinv_u, perm, v, tr);
  });
}
}  // namespace

MXLO_API int32_t mxlo_trisolve_mul(mxlo_ctx *ctx, int32_t dtype, void *res, const void *Tm, int64_t ld, int64_t n, int32_t upper,
                                   int32_t op_mode, const double *dinv, double *work, const void *v, double alpha, double beta) {
  return trisolve_mul(ctx, dtype, vectors(res, v, n, n), Tm, ld, n, upper, op_mode, dinv, work, alpha, beta, "mxlo_trisolve_mul");
}

MXLO_API int32_t mxlo_trisolve_mul_block(mxlo_ctx *ctx, int32_t dtype, void *res, int64_t ldr, const void *Tm, int64_t ld, int64_t n,
                                         int32_t upper, int32_t op_mode, const double *dinv, double *work, const void *V, int64_t ldv,
                                         int64_t k, double alpha, double beta) {
  return trisolve_mul(ctx, dtype, columns(res, ldr, V, ldv, k, n, n), Tm, ld, n, upper, op_mode, dinv, work, alpha, beta,
                      "mxlo_trisolve_mul_block");
}

MXLO_API int32_t mxlo_chol_mul(mxlo_ctx *ctx, int32_t dtype, void *res, const void *L, int64_t ld, int64_t n, const double *dinv,
                               double *work, const void *v, double alpha, double beta) {
  return sym_mul(ctx, dtype, vectors(res, v, n, n), L, ld, n, dinv, nullptr, false, work, alpha, beta, "mxlo_chol_mul");
}

MXLO_API int32_t mxlo_chol_mul_block(mxlo_ctx *ctx, int32_t dtype, void *res, int64_t ldr, const void *L, int64_t ld, int64_t n,
                                     const double *dinv, double *work, const void *V, int64_t ldv, int64_t k, double alpha,
                                     double beta) {
  return sym_mul(ctx, dtype, columns(res, ldr, V, ldv, k, n, n), L, ld, n, dinv, nullptr, false, work, alpha, beta, "mxlo_chol_mul_block");
}

MXLO_API int32_t mxlo_ldl_mul(mxlo_ctx *ctx, int32_t dtype, void *res, const void *L, int64_t ld, int64_t n, const double *dinv,
                              const double *d, double *work, const void *v, double alpha, double beta) {
  return sym_mul(ctx, dtype, vectors(res, v, n, n), L, ld, n, dinv, d, true, work, alpha, beta, "mxlo_ldl_mul");
}

MXLO_API int32_t mxlo_ldl_mul_block(mxlo_ctx *ctx, int32_t dtype, void *res, int64_t ldr, const void *L, int64_t ld, int64_t n,
                                    const double *dinv, const double *d, double *work, const void *V, int64_t ldv, int64_t k,
                                    double alpha, double beta) {
  return sym_mul(ctx, dtype, columns(res, ldr, V, ldv, k, n, n), L, ld, n, dinv, d, true, work, alpha, beta, "mxlo_ldl_mul_block");
}

MXLO_API int32_t mxlo_getrf(mxlo_ctx *ctx, int32_t dtype, const void *M, int64_t ldm, void *W, int64_t ldw, int64_t n, double *dinv_l,
                            double *dinv_u, int32_t *perm, int32_t *info_dev, int32_t *info) {
  const char *what = "mxlo_getrf";
  MXLO_TRY(check_common(ctx, dtype, W, ldw, n, what));
  MXLO_REQUIRE(info, MXLO_EINVAL, "%s: null info", what);
  *info = 0;
  if (n == 0) return MXLO_OK;
  MXLO_REQUIRE(dinv_l && dinv_u && perm && info_dev, MXLO_EINVAL, "%s: null storage for the block inverses / the permutation / the info word", what);
  MXLO_REQUIRE(n < (1LL << 31) - NB, MXLO_ESHAPE, "%s: n = %lld is too large", what, (long long)n);
  if (M) MXLO_REQUIRE(ldm >= (n > 1 ? n : 1), MXLO_ESHAPE, "%s: ldm = %lld < n", what, (long long)ldm);
  const int64_t es = esize(dtype);
  const Buf m{M, M ? mat_bytes(n, n, ldm, es) : 0, "M"};   // the permutation counts as 8 n bytes; the info word is held against M only
  MXLO_TRY(disjoint({m, {W, mat_bytes(n, n, ldw, es), "the factor"}, {dinv_l, blocks_bytes(n), "the block inverses of L"},
                     {dinv_u, blocks_bytes(n), "the block inverses of U"}, {perm, 8 * n, "the permutation"}}, what));
  MXLO_TRY(disjoint({m, {info_dev, 4, "the info word"}}, what));
  MXLO_TRY(refuse_capture(ctx, what));
  MXLO_DEVICE_GUARD(ctx);
  MXLO_TRY(with_real(dtype, [&]<typename T>() { return getrf_t<T>(ctx, (const T *)M, ldm, (T *)W, ldw, n, dinv_l, dinv_u, perm, info_dev); }));
  return read_back(ctx, info_dev, info, 1);
}

MXLO_API int32_t mxlo_lu_mul(mxlo_ctx *ctx, int32_t dtype, void *res, const void *W, int64_t ldw, int64_t n, const double *dinv_l,
                             const double *dinv_u, const int32_t *perm, double *work, const void *v, int32_t op_mode, double alpha,
                             double beta) {
  return lu_mul(ctx, dtype, vectors(res, v, n, n), W, ldw, n, dinv_l, dinv_u, perm, work, op_mode, alpha, beta, "mxlo_lu_mul");
}

MXLO_API int32_t mxlo_lu_mul_block(mxlo_ctx *ctx, int32_t dtype, void *res, int64_t ldr, const void *W, int64_t ldw, int64_t n,
                                   const double *dinv_l, const double *dinv_u, const int32_t *perm, double *work, const void *V,
                                   int64_t ldv, int64_t k, int32_t op_mode, double alpha, double beta) {
  return lu_mul(ctx, dtype, columns(res, ldr, V, ldv, k, n, n), W, ldw, n, dinv_l, dinv_u, perm, work, op_mode, alpha, beta,
                "mxlo_lu_mul_block");
}

// ---------------------------------------------------------------------------------------------- iterative refinement
// refine = r of opCholesky / opLDL / opLU: x_0 = F \ v, then r times x += F \ (v - op(M) x), with the residual and x in f64
// for both element types and ONE rounding to T, in the epilogue. A step is the chain of sweeps once more plus one residual
// launch; nothing is read back. The matrix the residual reads is a snapshot the operator took at construction: for the
// symmetric operators the strict upper triangle of M, parked in the strict upper triangle of the factor's storage W (which
// no factorisation or sweep kernel reads or writes: all of them guard with row >= column), and the diagonal in dg; for
// opLU a second n x n matrix A2 = P A, the stored matrix with its rows in pivot order. With A2 the iterate and the residual
// of a step live in the order the sweeps work in (N: A2 x = P v, only v is gathered; T: A' x = A2' y with y = P x the
// unscattered solution), so no launch permutes a vector in place and only the last epilogue scatters.
namespace {
constexpr int RLD = NB + 1;          // padded row of the transposed tile in LDS

// R[:, j] = V[:, j] - op(A) X[:, j], j < kb <= KB, in row bands of 64: workgroup b owns rows 64 b .. and walks the 64-wide
// chunks of the other index in ascending order. MODE 1: op(A) = A, the lanes run down the band's rows (unit stride).
// MODE 2: op(A) = A', the chunk's tile is loaded with unit stride and turned in LDS. MODE 0: A is the strict upper triangle
// U of a symmetric matrix with diagonal dg: chunks right of the band are read as in MODE 1 (U[band, chunk]), chunks left of
// it as in MODE 2 (U[chunk, band]'), the band's own tile both ways; only elements with row < column are loaded. Per (row,
// column j) the sum is 16-term fma chains per quarter of a chunk, carried over the chunks in order, then (p0 + p1) + (p2 +
// p3): fixed, independent of kb and of the other columns. Rows >= n and masked elements are never loaded.
template <typename T, int MODE>
__global__ void __launch_bounds__(kBlock) residual_kernel(const T *__restrict__ A, int64_t ld, const T *__restrict__ dg, int64_t n,
                                                          const T *__restrict__ V, int64_t ldv, const int *__restrict__ vgather,
                                                          const double *__restrict__ X, double *__restrict__ R, int kb) {
  __shared__ double sx[KB][NB], spart[KB][4][NB];
  __shared__ T st[NB][RLD];
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int b = blockIdx.x, nbk = gridDim.x;
  const int64_t i0 = (int64_t)b * NB;
  const int bl = (int)(n - i0 < NB ? n - i0 : NB);
  double acc[KB];
#pragma unroll
  for (int j = 0; j < KB; ++j) acc[j] = 0.0;
  for (int t = 0; t < nbk; ++t) {
    const int64_t c0 = (int64_t)t * NB;
    const int cl = (int)(n - c0 < NB ? n - c0 : NB);
    const int kind = MODE == 1 ? 0 : (MODE == 2 ? 1 : (t > b ? 0 : (t < b ? 1 : 2)));   // 0: direct, 1: turned, 2: the diagonal tile
    __syncthreads();                                     // the chunk before is consumed
    for (int e = tid; e < kb * NB; e += kBlock) {
      const int j = e >> 6, r = e & 63;
      sx[j][r] = r < cl ? X[c0 + r + (int64_t)j * n] : 0.0;
    }
    if (kind != 0) {                                     // st[cc][r] = A[c0 + r, i0 + cc]: row r of the chunk, column cc of the band
      for (int cc = q; cc < NB; cc += 4) {
        T x = T(0);
        if (lane < cl && cc < bl && (kind == 1 || lane < cc)) x = __builtin_nontemporal_load(A + (c0 + lane) + (i0 + cc) * ld);
        st[cc][lane] = x;
      }
    }
    __syncthreads();
    if (lane < bl) {
#pragma unroll
      for (int tt = 0; tt < 16; ++tt) {
        const int c = q * 16 + tt;
        if (c < cl) {
          double m;
          if (kind == 0) m = ld_stream(A + (i0 + lane) + (c0 + c) * ld);
          else if (kind == 1) m = (double)st[lane][c];
          else m = c > lane ? (double)st[c][lane] : (c < lane ? (double)st[lane][c] : (double)dg[i0 + lane]);
#pragma unroll
          for (int j = 0; j < KB; ++j)
            if (j < kb) acc[j] = fma(m, sx[j][c], acc[j]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < KB; ++j)
    if (j < kb) spart[j][q][lane] = acc[j];
  __syncthreads();
  if (tid < bl) {
    const int64_t i = i0 + tid;
    const int64_t src = vgather ? vgather[i] : i;
#pragma unroll
    for (int j = 0; j < KB; ++j)
      if (j < kb)
        R[i + (int64_t)j * n] = (double)V[src + (int64_t)j * ldv] -
                                ((spart[j][0][tid] + spart[j][1][tid]) + (spart[j][2][tid] + spart[j][3][tid]));
  }
}

template <typename T>
int32_t launch_residual(mxlo_ctx *ctx, int mode, const T *A, int64_t ld, const T *dg, int64_t n, const T *V, int64_t ldv,
                        const int *vgather, const double *X, double *R, int kb) {
  const dim3 grid((unsigned)((n + NB - 1) / NB)), blk(kBlock);
  if (mode == 0) hipLaunchKernelGGL((residual_kernel<T, 0>), grid, blk, 0, ctx->stream, A, ld, dg, n, V, ldv, vgather, X, R, kb);
  else if (mode == 1) hipLaunchKernelGGL((residual_kernel<T, 1>), grid, blk, 0, ctx->stream, A, ld, dg, n, V, ldv, vgather, X, R, kb);
  else hipLaunchKernelGGL((residual_kernel<T, 2>), grid, blk, 0, ctx->stream, A, ld, dg, n, V, ldv, vgather, X, R, kb);
  MXLO_LAUNCH_CHECK();
  return MXLO_OK;
}

// W[r, c] = M[r, c] for r < c and dg[i] = M[i, i], from the upper triangle of M (the one pack_upper_kernel reads); tiles
// below the diagonal return at once. A row-major M is turned through LDS so that both sides keep unit stride.
template <typename T>
__global__ void __launch_bounds__(kBlock) sym_snapshot_kernel(T *__restrict__ W, int64_t ldw, T *__restrict__ dg,
                                                              const T *__restrict__ M, int64_t ldm, int rowmajor, int64_t n) {
  if (blockIdx.x > blockIdx.y) return;                 // tile (br, bc) of W with br <= bc
  __shared__ T s[NB * (NB + 1)];
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * NB, c0 = (int64_t)blockIdx.y * NB;
  if (rowmajor) {                                      // M[r, c] = M[r * ldm + c]: unit stride along c
    for (int rl = q; rl < NB; rl += 4) {
      const int64_t r = r0 + rl, c = c0 + lane;
      s[rl * (NB + 1) + lane] = (r < n && c < n && r <= c) ? M[r * ldm + c] : T(0);
    }
    __syncthreads();
  }
  for (int cc = q; cc < NB; cc += 4) {
    const int64_t r = r0 + lane, c = c0 + cc;
    if (r < n && c < n && r <= c) {
      const T x = rowmajor ? s[lane * (NB + 1) + cc] : M[r + c * ldm];
      if (r < c) W[r + c * ldw] = x;
      else dg[r] = x;
    }
  }
}

// A2[i, c] = M[perm[i], c]: the stored matrix with its rows in pivot order
template <typename T>
__global__ void __launch_bounds__(kBlock) lu_snapshot_kernel(T *__restrict__ A2, int64_t lda, const T *__restrict__ M, int64_t ldm,
                                                             int64_t n, const int *__restrict__ perm) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t src = perm[i];
  for (int64_t c = blockIdx.y; c < n; c += gridDim.y) A2[i + c * lda] = M[src + c * ldm];
}

constexpr int MAX_STEPS = 8;         // linalg.py's MAX_REFINE

// what every refined apply adds to check_apply's: steps, the 2 n KB doubles of work, the snapshot's further storage
int32_t check_refine(int32_t dtype, const Operands &o, int64_t n, int32_t steps, const double *work, const Buf &snapshot, const char *what,
                     bool go) {
  MXLO_REQUIRE(steps >= 0 && steps <= MAX_STEPS, MXLO_EINVAL, "%s: steps = %d outside 0 .. %d", what, steps, MAX_STEPS);
  return go ? check_owned(dtype, o, {{work, 2 * n * KB * 8, "the work matrices"}, snapshot}, what) : MXLO_OK;
}

// one group of a refined apply: solve(v, xmode) runs the operator's chain of sweeps, resid() the residual launch
template <typename T, typename S, typename R>
int32_t refine_group(const T *v, int steps, S &&solve, R &&resid) {
  MXLO_TRY(solve(v, steps > 0 ? 1 : 0));
  for (int s = 1; s <= steps; ++s) {
    MXLO_TRY(resid());
    MXLO_TRY(solve((const T *)nullptr, s == steps ? 3 : 2));
  }
  return MXLO_OK;
}

template <typename T>
int32_t chol_refine_t(mxlo_ctx *ctx, T *res, int64_t ldr, const T *W, int64_t ld, int64_t n, const double *dinv, const double *d,
                      const T *dg, double *work, const T *V, int64_t ldv, int64_t k, int steps, double alpha, double beta) {
  double *z = work, *x = work + n * KB;
  return for_groups(res, ldr, V, ldv, k, [&](T *r, const T *v, Group grp) {
    return refine_group<T>(
        v, steps,
        [&](const T *rhs, int xmode) {
          return sym_mul_t<T>({.ctx = ctx, .res = r, .alpha = alpha, .beta = beta, .z = z, .grp = grp, .xacc = xmode ? x : nullptr, .xmode = xmode},
                              W, ld, n, dinv, d, rhs);
        },
        [&]() { return launch_residual<T>(ctx, 0, W, ld, dg, n, v, ldv, nullptr, x, z, grp.kb); });
  });
}

template <typename T>
int32_t lu_refine_t(mxlo_ctx *ctx, T *res, int64_t ldr, const T *W, int64_t ld, int64_t n, const double *dinv_l, const double *dinv_u,
                    const int *perm, const T *A2, int64_t lda, double *work, const T *V, int64_t ldv, int64_t k, int steps, bool trans,
                    double alpha, double beta) {
  double *z = work, *x = work + n * KB;
  return for_groups(res, ldr, V, ldv, k, [&](T *r, const T *v, Group grp) {
    return refine_group<T>(
        v, steps,
        [&](const T *rhs, int xmode) {
          return lu_mul_t<T>({.ctx = ctx, .res = r, .alpha = alpha, .beta = beta, .z = z, .grp = grp, .xacc = xmode ? x : nullptr, .xmode = xmode},
                             W, ld, n, dinv_l, dinv_u, perm, rhs, trans);
        },
        [&]() { return launch_residual<T>(ctx, trans ? 2 : 1, A2, lda, (const T *)nullptr, n, v, ldv, trans ? nullptr : perm, x, z, grp.kb); });
  });
}

int32_t sym_refine(mxlo_ctx *ctx, int32_t dtype, void *res, int64_t ldr, const void *W, int64_t ldw, int64_t n, const double *dinv,
                   const double *d, const void *dg, double *work, const void *V, int64_t ldv, int64_t k, int32_t steps, double alpha,
                   double beta, bool ldl, const char *what) {
  const Operands o = columns(res, ldr, V, ldv, k, n, n);
  bool go;
  MXLO_TRY(check_apply(ctx, dtype, o, W, ldw, n, dinv, work, what, go));
  if (ldl && go) MXLO_TRY(check_owned(dtype, o, {{d, n * 8, "the pivots"}}, what));
  MXLO_TRY(check_refine(dtype, o, n, steps, work, {dg, n * esize(dtype), "the diagonal of the snapshot"}, what, go));
  if (!go) return MXLO_OK;
  MXLO_DEVICE_GUARD(ctx);
  return with_real(dtype, [&]<typename T>() {
    return chol_refine_t<T>(ctx, (T *)res, ldr, (const T *)W, ldw, n, dinv, d, (const T *)dg, work, (const T *)V, ldv, k, steps, alpha, beta);
  });
}

}  // namespace

MXLO_API int32_t mxlo_sym_snapshot(mxlo_ctx *ctx, int32_t dtype, const void *M, int64_t ldm, int32_t m_rowmajor, void *W, int64_t ldw,
                                   int64_t n, void *dg) {
  const char *what = "mxlo_sym_snapshot";
  MXLO_TRY(check_common(ctx, dtype, W, ldw, n, what));
  if (n == 0) return MXLO_OK;
  MXLO_REQUIRE(M && dg && ldm >= (n > 1 ? n : 1), MXLO_EINVAL, "%s: null operand or ldm = %lld < n", what, (long long)ldm);
  MXLO_REQUIRE(n < (1LL << 31) - NB, MXLO_ESHAPE, "%s: n = %lld is too large", what, (long long)n);
  const int64_t es = esize(dtype);
  MXLO_TRY(disjoint({{M, mat_bytes(n, n, ldm, es), "M"}, {W, mat_bytes(n, n, ldw, es), "the factor"}, {dg, n * es, "the diagonal vector"}},
                    what));
  MXLO_DEVICE_GUARD(ctx);
  const unsigned nb = (unsigned)((n + NB - 1) / NB);
  return with_real(dtype, [&]<typename T>() -> int32_t {
    hipLaunchKernelGGL((sym_snapshot_kernel<T>), dim3(nb, nb), dim3(kBlock), 0, ctx->stream, (T *)W, ldw, (T *)dg, (const T *)M, ldm,
                       m_rowmajor ? 1 : 0, n);
    MXLO_LAUNCH_CHECK();
    return MXLO_OK;
  });
}

MXLO_API int32_t mxlo_lu_snapshot(mxlo_ctx *ctx, int32_t dtype, const void *M, int64_t ldm, const int32_t *perm, void *A2, int64_t lda,
                                  int64_t n) {
  const char *what = "mxlo_lu_snapshot";
  MXLO_TRY(check_common(ctx, dtype, A2, lda, n, what));
  if (n == 0) return MXLO_OK;
  MXLO_REQUIRE(M && perm && ldm >= (n > 1 ? n : 1), MXLO_EINVAL, "%s: null operand or ldm = %lld < n", what, (long long)ldm);
  MXLO_REQUIRE(n < (1LL << 31) - NB, MXLO_ESHAPE, "%s: n = %lld is too large", what, (long long)n);
  const int64_t es = esize(dtype);
  MXLO_TRY(apart({A2, mat_bytes(n, n, lda, es), "the snapshot"}, {{M, mat_bytes(n, n, ldm, es), "M"}, {perm, n * 4, "the permutation"}}, what));
  MXLO_DEVICE_GUARD(ctx);
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock), (unsigned)(n < 1024 ? n : 1024));
  return with_real(dtype, [&]<typename T>() -> int32_t {
    hipLaunchKernelGGL((lu_snapshot_kernel<T>), grid, dim3(kBlock), 0, ctx->stream, (T *)A2, lda, (const T *)M, ldm, n, perm);
    MXLO_LAUNCH_CHECK();
    return MXLO_OK;
  });
}

namespace {
// R and X of a residual entry point: n x k doubles with column stride n, k <= KB; R may overlap nothing it reads
int32_t check_residual(mxlo_ctx *ctx, int32_t dtype, const double *R, const void *A, int64_t ld, const void *dg, int64_t n, const void *V,
                       int64_t ldv, const double *X, int64_t k, const char *what) {
  MXLO_TRY(check_common(ctx, dtype, A, ld, n, what));
  MXLO_REQUIRE(k >= 0 && k <= KB && ldv >= (n > 1 ? n : 1), MXLO_ESHAPE, "%s: k = %lld (at most %d), ldv = %lld", what, (long long)k, KB,
               (long long)ldv);
  if (n == 0 || k == 0) return MXLO_OK;
  MXLO_REQUIRE(R && V && X, MXLO_EINVAL, "%s: null operand", what);
  MXLO_REQUIRE(n < (1LL << 31) - NB, MXLO_ESHAPE, "%s: n = %lld is too large", what, (long long)n);
  const int64_t es = esize(dtype);
  return apart({R, n * k * 8, "R"},
               {{X, n * k * 8, "X"}, {V, mat_bytes(n, k, ldv, es), "V"}, {A, mat_bytes(n, n, ld, es), "the matrix"}, {dg, n * es, "the diagonal"}},
               what);
}
}  // namespace

MXLO_API int32_t mxlo_sym_residual(mxlo_ctx *ctx, int32_t dtype, double *R, const void *U, int64_t ld, const void *dg, int64_t n,
                                   const void *V, int64_t ldv, const double *X, int64_t k) {
  MXLO_TRY(check_residual(ctx, dtype, R, U, ld, dg, n, V, ldv, X, k, "mxlo_sym_residual"));
  if (n == 0 || k == 0) return MXLO_OK;
  MXLO_REQUIRE(dg, MXLO_EINVAL, "mxlo_sym_residual: null diagonal");
  MXLO_DEVICE_GUARD(ctx);
  return with_real(dtype, [&]<typename T>() {
    return launch_residual<T>(ctx, 0, (const T *)U, ld, (const T *)dg, n, (const T *)V, ldv, nullptr, X, R, (int)k);
  });
}

MXLO_API int32_t mxlo_gen_residual(mxlo_ctx *ctx, int32_t dtype, double *R, const void *A, int64_t ld, int64_t n, const void *V,
                                   int64_t ldv, const double *X, int64_t k, int32_t op_mode) {
  MXLO_TRY(check_residual(ctx, dtype, R, A, ld, nullptr, n, V, ldv, X, k, "mxlo_gen_residual"));
  MXLO_TRY(check_mode(op_mode, "mxlo_gen_residual"));
  if (n == 0 || k == 0) return MXLO_OK;
  MXLO_DEVICE_GUARD(ctx);
  const int mode = op_mode == MXLO_OP_N ? 1 : 2;
  return with_real(dtype, [&]<typename T>() {
    return launch_residual<T>(ctx, mode, (const T *)A, ld, (const T *)nullptr, n, (const T *)V, ldv, nullptr, X, R, (int)k);
  });
}

MXLO_API int32_t mxlo_chol_mul_refine(mxlo_ctx *ctx, int32_t dtype, void *res, int64_t ldr, const void *W, int64_t ldw, int64_t n,
                                      const double *dinv, const void *dg, double *work, const void *V, int64_t ldv, int64_t k,
                                      int32_t steps, double alpha, double beta) {
  return sym_refine(ctx, dtype, res, ldr, W, ldw, n, dinv, nullptr, dg, work, V, ldv, k, steps, alpha, beta, false, "mxlo_chol_mul_refine");
}

MXLO_API int32_t mxlo_ldl_mul_refine(mxlo_ctx *ctx, int32_t dtype, void *res, int64_t ldr, const void *W, int64_t ldw, int64_t n,
                                     const double *dinv, const double *d, const void *dg, double *work, const void *V, int64_t ldv,
                                     int64_t k, int32_t steps, double alpha, double beta) {
  return sym_refine(ctx, dtype, res, ldr, W, ldw, n, dinv, d, dg, work, V, ldv, k, steps, alpha, beta, true, "mxlo_ldl_mul_refine");
}

MXLO_API int32_t mxlo_lu_mul_refine(mxlo_ctx *ctx, int32_t dtype, void *res, int64_t ldr, const void *W, int64_t ldw, int64_t n,
                                    const double *dinv_l, const double *dinv_u, const int32_t *perm, const void *A2, int64_t lda,
                                    double *work, const void *V, int64_t ldv, int64_t k, int32_t steps, int32_t op_mode, double alpha,
                                    double beta) {
  const char *what = "mxlo_lu_mul_refine";
  const Operands o = columns(res, ldr, V, ldv, k, n, n);
  bool go;
  MXLO_TRY(check_lu_apply(ctx, dtype, o, W, ldw, n, dinv_l, dinv_u, perm, work, what, go));
  MXLO_TRY(check_mode(op_mode, what));
  MXLO_REQUIRE(lda >= (n > 1 ? n : 1), MXLO_ESHAPE, "%s: lda = %lld < n", what, (long long)lda);
  MXLO_TRY(check_refine(dtype, o, n, steps, work, {A2, mat_bytes(n, n, lda, esize(dtype)), "the snapshot"}, what, go));
  if (!go) return MXLO_OK;
  MXLO_DEVICE_GUARD(ctx);
  const bool tr = op_mode != MXLO_OP_N;
  return with_real(dtype, [&]<typename T>() {
    return lu_refine_t<T>(ctx, (T *)res, ldr, (const T *)W, ldw, n, dinv_l, dinv_u, perm, (const T *)A2, lda, work, (const T *)V, ldv, k, steps,
                          tr, alpha, beta);
  });
}

// ---------------------------------------------------------------------------------------------- geqrf / qr_mul
// opQR (src/linalg.jl:3-9, 27-32 for a rectangular dense M): F = Q R of the TALL orientation F (mf x nf, mf >= nf) by unpivoted
// Householder reflections in block columns of NB, LAPACK's layout (R on and above the diagonal of W, the reflector vectors
// below it with an implicit unit first entry) with one NB x NB compact-WY factor T per block column, Q_k = I - V_k T_k V_k'.
// Rows are cut into chunks of NB dealt round-robin to at most QG workgroups. A pass over a tall panel leaves one partial
// sum per workgroup and column; the NEXT launch's workgroups each add them up in the same fixed order, so nothing but the
// launch boundary orders the workgroups, and the grid and the order of every sum depend on the shape only.
namespace {

constexpr int QG = 512;              // most workgroups of a pass over the rows = partial slots per column

inline int qr_grid(int64_t rows) {
  const int64_t ch = (rows + NB - 1) / NB;
  return (int)(ch < 1 ? 1 : (ch < QG ? ch : QG));
}

// quarter q of the sum below: part[g * NB + lane] over g = q, q + 4, .. < G, in that order
__device__ __forceinline__ double qr_quarter(const double *__restrict__ part, int G, int lane, int q) {
  double acc = 0.0;
  int g = q;
  for (; g + 28 < G; g += 32) {                          // eight independent loads in flight, added in the order of the plain loop
    double p[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) p[t] = part[(int64_t)(g + 4 * t) * NB + lane];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc += p[t];
  }
  for (; g < G; g += 4) acc += part[(int64_t)g * NB + lane];
  return acc;
}

// s[c] = sum over g < G of part[g * NB + c]: four strided quarters, then (p0 + p1) + (p2 + p3)
__device__ __forceinline__ void qr_reduce(const double *__restrict__ part, int G, double *s, double (*spart)[NB], int lane, int q) {
  spart[q][lane] = qr_quarter(part, G, lane, q);
  __syncthreads();
  if (q == 0) s[lane] = (spart[0][lane] + spart[1][lane]) + (spart[2][lane] + spart[3][lane]);
  __syncthreads();
}

// W = F: M as it lies (column-major mf x nf), or — trans — M is the column-major nf x mf storage of F', turned through LDS
template <typename T>
__global__ void __launch_bounds__(kBlock) qr_copy_kernel(T *__restrict__ W, int64_t ldw, const T *__restrict__ M, int64_t ldm, int trans,
                                                         int64_t mf, int64_t nf) {
  __shared__ T s[NB * (NB + 1)];
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * NB, c0 = (int64_t)blockIdx.y * NB;
  if (!trans) {
    for (int cl = q; cl < NB; cl += 4) {
      const int64_t i = i0 + lane, c = c0 + cl;
      if (i < mf && c < nf) W[i + c * ldw] = M[i + c * ldm];
    }
    return;
  }
  for (int il = q; il < NB; il += 4) {                 // F[i, c] = M[c + i * ldm]: unit stride along c
    const int64_t i = i0 + il, c = c0 + lane;
    s[il * (NB + 1) + lane] = (i < mf && c < nf) ? M[c + i * ldm] : T(0);
  }
  __syncthreads();
  for (int cl = q; cl < NB; cl += 4) {
    const int64_t i = i0 + lane, c = c0 + cl;
    if (i < mf && c < nf) W[i + c * ldw] = s[lane * (NB + 1) + cl];
  }
}

// phase (a), one launch per panel column c = -1 .. jb - 1 over all row chunks of the panel (rows j0 .. mf, columns j0 .. j0 + jb).
// Launch c (>= 0) first adds up what launch c - 1 left: pin, the dots of column c with every column of the panel over the rows
// strictly below its diagonal row d = j0 + c, and din, row d itself. From those alone every workgroup has the reflector of
// column c in larfg's convention — beta = -sign(alpha) |(alpha, x)|, tau = (beta - alpha) / beta, v = x / (alpha - beta);
// x == 0: tau = 0, H = I — and w_j = tau v' a_j for the later columns; workgroup 0 also writes column c of T,
// T[0:c, c] = -tau T[0:c, 0:c] (V[:, 0:c]' v), T[c, c] = tau. Then every workgroup turns its rows of column c into v, applies
// a_j -= w_j v to its rows of the later columns, and (c + 1 < jb) leaves pout / dout for column c + 1. Launch -1 only does the
// latter, for column 0. A column whose norm from the diagonal down is zero or not finite stores its 1-based index in *info.
template <typename T>
__global__ void __launch_bounds__(kBlock) geqrf_panel_kernel(T *W, int64_t ldw, int64_t mf, int64_t j0, int jb, int c,
                                                             double *tfac, const double *__restrict__ pin,
                                                             const double *__restrict__ din, double *__restrict__ pout,
                                                             double *__restrict__ dout, int *info) {
  __shared__ double sS[NB], sD[NB], sW[NB], spart[4][NB];
  if (*info != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int g = blockIdx.x, G = gridDim.x;
  const int cn = c + 1 < jb ? c + 1 : -1;
  const int64_t d = j0 + c, dn = j0 + cn;
  double scale = 0.0, beta = 0.0;
  if (c >= 0) {
    qr_reduce(pin, G, sS, spart, lane, q);
    if (tid < NB) sD[tid] = din[tid];
    __syncthreads();
    const double alpha = sD[c], sigma = sS[c];
    const double nrm = sqrt(fma(alpha, alpha, sigma));
    if (nrm == 0.0 || !(nrm < __builtin_inf())) {        // the same value in every thread of every workgroup
      if (g == 0 && tid == 0) *info = (int)(d + 1);
      return;
    }
    double tau = 0.0;
    beta = alpha;
    if (sigma != 0.0) {
      beta = -copysign(nrm, alpha);
      tau = (beta - alpha) / beta;
      scale = 1.0 / (alpha - beta);
    }
    if (tid < NB) sW[tid] = (tid > c && tid < jb) ? tau * fma(scale, sS[tid], sD[tid]) : 0.0;
    if (g == 0) {
      if (tid < NB) spart[0][tid] = tid < c ? fma(scale, sS[tid], sD[tid]) : 0.0;     // V[:, i]' v, i < c
      __syncthreads();
      if (tid < NB) {
        double t = 0.0;
        if (tid < c) {
#pragma unroll 8
          for (int l = tid; l < c; ++l) t = fma(tfac[tid + l * NB], spart[0][l], t);
          t = -tau * t;
        } else if (tid == c) t = tau;
        tfac[tid + c * NB] = t;
      }
    }
    __syncthreads();
  }
  T *P = W + j0 * ldw;
  const int64_t nch = (mf - j0 + NB - 1) / NB;
  double acc[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = 0.0;
  for (int64_t ch = g; ch < nch; ch += G) {
    const int64_t r = j0 + ch * NB + lane;
    const bool in = r < mf;
    double xr = 0.0, yr = 0.0, val[16];
    if (c >= 0 && in && r > d) xr = (double)P[r + c * ldw];
    if (cn >= 0 && in) yr = (double)P[r + cn * ldw];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int j = q * 16 + t;
      val[t] = (in && j < jb) ? (double)P[r + j * ldw] : 0.0;
    }
    __syncthreads();                                     // columns c and c + 1 are read by every wave before their owners write them
    if (c >= 0 && in && r >= d) {
      const double vr = r > d ? (double)(T)(xr * scale) : 1.0;
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int j = q * 16 + t;
        if (j >= c && j < jb) {
          const T x = j > c ? (T)fma(-sW[j], vr, val[t]) : (r > d ? (T)vr : (T)beta);
          P[r + j * ldw] = x;
          val[t] = j > c ? (double)x : vr;
        }
      }
      if (cn >= 0) yr = (double)(T)fma(-sW[cn], vr, yr);
    }
    if (cn >= 0) {
      if (in && r > dn) {
#pragma unroll
        for (int t = 0; t < 16; ++t) acc[t] = fma(val[t], yr, acc[t]);
      }
      if (r == dn) {
#pragma unroll
        for (int t = 0; t < 16; ++t) dout[q * 16 + t] = val[t];
      }
    }
  }
  if (cn >= 0) {
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const double s = wave_sum(acc[t]);
      if (lane == 0) pout[(int64_t)g * NB + q * 16 + t] = s;
    }
  }
}

// phase (c), step 1: partial Y = V' C over the rows [k_lo, k_hi) of split blockIdx.y, one 64 x 64 tile of columns of C per
// blockIdx.x, on the MFMA of the element type. V is the panel with its implicit unit diagonal and zeros above it.
template <typename T>
__global__ void __launch_bounds__(kBlock) geqrf_vtc_kernel(const T *__restrict__ V, const T *__restrict__ Cm, int64_t ld, int64_t rows,
                                                           int jb, int nc, int64_t rs, double *__restrict__ ypart, const int *info) {
  if (*info != 0) return;
  __shared__ T sA[SK][SLD], sB[SK][SLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bn = blockIdx.x * NB;
  const int64_t k_lo = (int64_t)blockIdx.y * rs, k_hi = k_lo + rs < rows ? k_lo + rs : rows;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  using Acc = typename Mfma<T>::Acc;
  Acc acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[a][b][r] = 0;
  for (int64_t k0 = k_lo; k0 < k_hi; k0 += SK) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int e = tid + t * kBlock, kb = e & 15, col = e >> 4;
      const int64_t gk = k0 + kb;
      T va = T(0);
      if (gk < k_hi && col < jb) va = gk > col ? V[gk + (int64_t)col * ld] : (gk == col ? T(1) : T(0));
      sA[kb][col] = va;
      sB[kb][col] = (gk < k_hi && bn + col < nc) ? Cm[gk + (int64_t)(bn + col) * ld] : T(0);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < SK; kk += 4) {
      const int kr = kk + (lane >> 4);
      const T a0 = sA[kr][wm + (lane & 15)], a1 = sA[kr][wm + 16 + (lane & 15)];
      const T b0 = sB[kr][wn + (lane & 15)], b1 = sB[kr][wn + 16 + (lane & 15)];
      acc[0][0] = Mfma<T>::run(a0, b0, acc[0][0]);
      acc[0][1] = Mfma<T>::run(a0, b1, acc[0][1]);
      acc[1][0] = Mfma<T>::run(a1, b0, acc[1][0]);
      acc[1][1] = Mfma<T>::run(a1, b1, acc[1][1]);
    }
    __syncthreads();
  }
  double *out = ypart + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * NB2;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = wm + a * 16 + Mfma<T>::row(lane, r), gj = wn + b * 16 + (lane & 15);
        out[gj * NB + gi] = (double)acc[a][b][r];
      }
}

// step 2: Y = T' (sum of the S partial tiles, in order), f64, stored in the element type for step 3; one workgroup a tile
template <typename T>
__global__ void __launch_bounds__(kBlock) geqrf_ty_kernel(const double *__restrict__ ypart, int S, const double *__restrict__ tfac, int jb,
                                                          T *__restrict__ y2, const int *info) {
  if (*info != 0) return;
  __shared__ double sY[NB * (NB + 1)];
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  for (int e = tid; e < NB2; e += kBlock) {
    double a = 0.0;
    for (int s = 0; s < S; ++s) a += ypart[((int64_t)s * gridDim.x + blockIdx.x) * NB2 + e];
    sY[(e >> 6) * (NB + 1) + (e & 63)] = a;
  }
  __syncthreads();
  T *out = y2 + (int64_t)blockIdx.x * NB2;
  for (int i = q; i < NB; i += 4) {                      // row i of T' Y, the lanes across the columns of the tile
    double a = 0.0;
    if (i < jb)
      for (int l = 0; l <= i; ++l) a = fma(tfac[l + i * NB], sY[lane * (NB + 1) + l], a);
    out[lane * NB + i] = (T)a;
  }
}

// step 3: C -= V Y, the rank-jb update of getrf_gemm_kernel with V's implicit unit diagonal and a rectangular C (rows x nc)
template <typename T>
__global__ void __launch_bounds__(kBlock) geqrf_update_kernel(T *__restrict__ Cm, const T *__restrict__ V, const T *__restrict__ y2,
                                                              int64_t ld, int64_t rows, int jb, int nc, const int *info) {
  if (*info != 0) return;
  __shared__ T sA[SK][SLD], sB[SK][SLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t bm = (int64_t)blockIdx.x * NB;
  const int bn = blockIdx.y * NB;
  const T *Yt = y2 + (int64_t)blockIdx.y * NB2;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  using Acc = typename Mfma<T>::Acc;
  Acc acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[a][b][r] = 0;
  for (int k0 = 0; k0 < jb; k0 += SK) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int e = tid + t * kBlock, i = e & 63, k = e >> 6, kb = e & 15, jn = e >> 4;
      const int64_t gi = bm + i;
      const int gk = k0 + k;
      T va = T(0);
      if (gi < rows && gk < jb) va = gi > gk ? V[gi + (int64_t)gk * ld] : (gi == gk ? T(1) : T(0));
      sA[k][i] = va;
      sB[kb][jn] = k0 + kb < jb ? Yt[jn * NB + k0 + kb] : T(0);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < SK; kk += 4) {
      const int kr = kk + (lane >> 4);
      const T a0 = sA[kr][wm + (lane & 15)], a1 = sA[kr][wm + 16 + (lane & 15)];
      const T b0 = sB[kr][wn + (lane & 15)], b1 = sB[kr][wn + 16 + (lane & 15)];
      acc[0][0] = Mfma<T>::run(a0, b0, acc[0][0]);
      acc[0][1] = Mfma<T>::run(a0, b1, acc[0][1]);
      acc[1][0] = Mfma<T>::run(a1, b0, acc[1][0]);
      acc[1][1] = Mfma<T>::run(a1, b1, acc[1][1]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t gi = bm + wm + a * 16 + Mfma<T>::row(lane, r);
        const int gj = bn + wn + b * 16 + (lane & 15);
        if (gi < rows && gj < nc) {
          T *p = Cm + gi + (int64_t)gj * ld;
          *p = *p - acc[a][b][r];
        }
      }
}

// doubles of mxlo_geqrf's scratch: two sets of partial slots and of the diagonal row, the partial tiles of V' C (at most
// max(512, tiles) of them) and the tiles of T' V' C
inline int64_t geqrf_scratch(int64_t nf) {
  const int64_t nb = (nf + NB - 1) / NB;
  return 2 * (int64_t)QG * NB + 2 * NB + (512 + 2 * nb) * NB2;
}

template <typename T>
int32_t geqrf_chain_t(mxlo_ctx *ctx, T *W, int64_t ldw, int64_t mf, int64_t nf, double *tfac, double *dinv, double *fwork, int *info_dev);

template <typename T>
int32_t geqrf_t(mxlo_ctx *ctx, const T *M, int64_t ldm, int trans, T *W, int64_t ldw, int64_t mf, int64_t nf, double *tfac, double *dinv,
                double *fwork, int *info_dev) {
  const int64_t nb = (nf + NB - 1) / NB;
  MXLO_HIP(hipMemsetAsync(info_dev, 0, sizeof(int), ctx->stream));
  hipLaunchKernelGGL((qr_copy_kernel<T>), dim3((unsigned)((mf + NB - 1) / NB), (unsigned)nb), dim3(kBlock), 0, ctx->stream, W, ldw, M, ldm,
                     trans, mf, nf);
  MXLO_LAUNCH_CHECK();
  return geqrf_chain_t<T>(ctx, W, ldw, mf, nf, tfac, dinv, fwork, info_dev);
}

// geqrf_t once W holds F and *info_dev is zero: the panels, the trailing updates and the block inverses of R
template <typename T>
int32_t geqrf_chain_t(mxlo_ctx *ctx, T *W, int64_t ldw, int64_t mf, int64_t nf, double *tfac, double *dinv, double *fwork, int *info_dev) {
  const int64_t nb = (nf + NB - 1) / NB;
  double *pb[2] = {fwork, fwork + (int64_t)QG * NB}, *db[2] = {fwork + 2 * (int64_t)QG * NB, fwork + 2 * (int64_t)QG * NB + NB};
  double *ypart = fwork + 2 * (int64_t)QG * NB + 2 * NB;
  for (int64_t k = 0; k < nb; ++k) {
    const int64_t j0 = k * NB, jb = nf - j0 < NB ? nf - j0 : NB, j1 = j0 + jb, nc = nf - j1, rows = mf - j0;
    const unsigned G = (unsigned)qr_grid(rows);
    for (int c = -1; c < (int)jb; ++c) {                 // launch c reads the slots c & 1 and leaves the others for launch c + 1
      hipLaunchKernelGGL((geqrf_panel_kernel<T>), dim3(G), dim3(kBlock), 0, ctx->stream, W, ldw, mf, j0, (int)jb, c, tfac + k * NB2,
                         (const double *)pb[c & 1], (const double *)db[c & 1], pb[(c + 1) & 1], db[(c + 1) & 1], info_dev);
      MXLO_LAUNCH_CHECK();
    }
    if (nc <= 0) break;
    const int64_t tiles = (nc + NB - 1) / NB, rch = (rows + NB - 1) / NB;
    int64_t S = 512 / tiles;
    S = S < 1 ? 1 : (S > rch ? rch : S);
    const int64_t rs = ((rows + S - 1) / S + SK - 1) / SK * SK;
    T *y2 = (T *)(ypart + S * tiles * NB2);
    const T *V = W + j0 + j0 * ldw;
    T *Cm = W + j0 + j1 * ldw;
    hipLaunchKernelGGL((geqrf_vtc_kernel<T>), dim3((unsigned)tiles, (unsigned)S), dim3(kBlock), 0, ctx->stream, V, (const T *)Cm, ldw, rows,
                       (int)jb, (int)nc, rs, ypart, (const int *)info_dev);
    MXLO_LAUNCH_CHECK();
    hipLaunchKernelGGL((geqrf_ty_kernel<T>), dim3((unsigned)tiles), dim3(kBlock), 0, ctx->stream, (const double *)ypart, (int)S,
                       (const double *)(tfac + k * NB2), (int)jb, y2, (const int *)info_dev);
    MXLO_LAUNCH_CHECK();
    hipLaunchKernelGGL((geqrf_update_kernel<T>), dim3((unsigned)rch, (unsigned)tiles), dim3(kBlock), 0, ctx->stream, Cm, V, (const T *)y2,
                       ldw, rows, (int)jb, (int)nc, (const int *)info_dev);
    MXLO_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL((tri_prepare_kernel<T>), dim3((unsigned)nb), dim3(kBlock), 0, ctx->stream, (const T *)W, ldw, nf, 1, dinv);   // phase (b)
  MXLO_LAUNCH_CHECK();
  return MXLO_OK;
}

// One launch of the reflector chain of an apply. It (1) adds up the partial dots d = V_p' z the launch before left and takes
// w = T_p' d (Q') or T_p d (Q), (2) z -= V_p w on its rows, (3) leaves the partial dots of the new z with V_n. The first launch
// of a chain has no block p and fills z (load 1: from v; 2: z below row nf is zero), the last has no block n and, with epi,
// writes res = alpha z + beta res instead of z. The panels are streamed; a panel is read by the launch that takes its dots and again
// by the next one, which applies it.
struct QrArgs {
  const void *W;
  int64_t ld, mf, nf;
  double *z;
  const void *v;
  int load;
  int64_t jp, jn;        // first column of the block applied / dotted against
  int jbp, jbn;          // their widths; 0: none
  const double *tp;      // T of block p, applied transposed if tp_trans
  int tp_trans;
  const double *pin;
  double *pout;
  int epi;
  void *res;
  double alpha, beta;
  int kb;                // block form (qr_reflect_block_kernel): the group's right-hand sides, 1 .. KB; 0: the vector kernel. v and
  int64_t ldr, ldv;      // res are then matrices with these leading dimensions, z is mf x kb with column stride mf, and right-hand
  double *zc;            // side j has its partial slots at pin / pout + j QG NB. zc: the sweep's compact nf x kb matrix (column stride
  int zc_out;            // nf), which load 2 reads rows < nf from and which the launch with zc_out writes them to instead of z
  const int *fill_idx;   // pivoted form, or NULL: this launch also writes res[fill_idx[i]] = alpha 0 + beta res[..] for fill_lo <= i <
  int64_t fill_lo, fill_hi;      // fill_hi, the entries of a rank-deficient solution that are no pivots (every column of a group)
  const int *idx;        // opPinv, or NULL: the launch with load 1 reads row r of z from v[idx[r]], the one with epi writes it to
};                       // res[idx[r]]; read once per chunk of rows, outside the loops over the columns. Such a launch runs the IDX
                         // instantiation of its kernel; the others run the code they ran before there was an idx

template <typename T, bool BETA0, bool IDX>
__global__ void __launch_bounds__(kBlock) qr_reflect_kernel(QrArgs a) {
  __shared__ double sd[NB], sw[NB], spart[4][NB], sT[NB * (NB + 1)];
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int g = blockIdx.x, G = gridDim.x;
  const T *W = (const T *)a.W;
  if (a.jbp) {
    for (int e = tid; e < NB2; e += kBlock) sT[(e >> 6) * (NB + 1) + (e & 63)] = a.tp[e];      // T[i, l] at sT[l * (NB + 1) + i]
    qr_reduce(a.pin, G, sd, spart, lane, q);
    double part = 0.0;                                   // T is upper triangular and zero outside its jbp columns: all 64 terms
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int l = q * 16 + t;
      part = fma(a.tp_trans ? sT[lane * (NB + 1) + l] : sT[l * (NB + 1) + lane], sd[l], part);
    }
    spart[q][lane] = part;
    __syncthreads();
    if (q == 0) sw[lane] = (spart[0][lane] + spart[1][lane]) + (spart[2][lane] + spart[3][lane]);
    __syncthreads();
  }
  double acc[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = 0.0;
  const int64_t nch = (a.mf + NB - 1) / NB;
  for (int64_t ch = g; ch < nch; ch += G) {
    const int64_t r = ch * NB + lane;
    const bool in = r < a.mf;
    double zr = 0.0;
    if (in) zr = a.load == 1 ? (double)((const T *)a.v)[IDX ? (int64_t)a.idx[r] : r] : ((a.load == 2 && r >= a.nf) ? 0.0 : a.z[r]);
    if (a.jbp) {
      double part = 0.0;
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int c = q * 16 + t;
        const int64_t col = a.jp + c;
        if (c < a.jbp && in && r >= col) part = fma(r > col ? ld_stream(W + r + col * a.ld) : 1.0, sw[c], part);
      }
      spart[q][lane] = part;
      __syncthreads();
      zr -= (spart[0][lane] + spart[1][lane]) + (spart[2][lane] + spart[3][lane]);
      __syncthreads();
    }
    if (q == 0 && in) {
      if (a.epi) store_res<T, BETA0>((T *)a.res, IDX ? (int64_t)a.idx[r] : r, zr, a.alpha, a.beta);
      else a.z[r] = zr;
    }
    if (a.jbn) {
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int c = q * 16 + t;
        const int64_t col = a.jn + c;
        if (c < a.jbn && in && r >= col) acc[t] = fma(r > col ? ld_stream(W + r + col * a.ld) : 1.0, zr, acc[t]);
      }
    }
  }
  if (a.jbn) {
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const double s = wave_sum(acc[t]);
      if (lane == 0) a.pout[(int64_t)g * NB + q * 16 + t] = s;
    }
  }
  if (a.fill_idx)
    for (int64_t i = a.fill_lo + (int64_t)g * kBlock + tid; i < a.fill_hi; i += (int64_t)G * kBlock)
      store_res<T, BETA0>((T *)a.res, a.fill_idx[i], 0.0, a.alpha, a.beta);
}

template <typename T>
int32_t launch_reflect(mxlo_ctx *ctx, const QrArgs &a) {
  const unsigned G = (unsigned)qr_grid(a.mf);
  if (a.idx) {
    if (a.beta == 0.0) hipLaunchKernelGGL((qr_reflect_kernel<T, true, true>), dim3(G), dim3(kBlock), 0, ctx->stream, a);
    else hipLaunchKernelGGL((qr_reflect_kernel<T, false, true>), dim3(G), dim3(kBlock), 0, ctx->stream, a);
  } else if (a.beta == 0.0) hipLaunchKernelGGL((qr_reflect_kernel<T, true, false>), dim3(G), dim3(kBlock), 0, ctx->stream, a);
  else hipLaunchKernelGGL((qr_reflect_kernel<T, false, false>), dim3(G), dim3(kBlock), 0, ctx->stream, a);
  MXLO_LAUNCH_CHECK();
  return MXLO_OK;
}

// qr_reflect_kernel carrying a group of kb <= KB right-hand sides, in a workgroup of 16 waves. Per right-hand side the
// operations and their order are the vector kernel's (qr_quarter and (p0 + p1) + (p2 + p3) for the slots, the four 16-term fma
// chains for w = T d and for z -= V w, one fma chain per (row, column) over the workgroup's chunks for the new dots, then
// wave_sum with the rows in the lanes), so column j is the vector apply of column j bit for bit. What is shared: every element
// of the chunk of V_p and of V_n is loaded from memory ONCE, by thread (row = lane, columns 4 wv .. 4 wv + 3), all at the top of
// the chunk — the chunk of V_p into LDS, that of V_n into four registers —, and the barriers of a chunk are paid once.
//   update (and the prologue): wave wv holds quarter q = wv & 3 of the right-hand sides 2 (wv >> 2), + 1; it reads V_p from LDS.
//   dots: thread (lane, wv) holds its 4 columns x KB right-hand sides: 32 accumulators, where 16 columns x KB would be 128.
//   z: wave j < kb holds z of right-hand side j for the chunk's rows and passes it to the dots through LDS.
constexpr int QBT = 1024;            // threads of qr_reflect_block_kernel

template <typename T, bool BETA0, bool IDX>
__global__ void __launch_bounds__(QBT) qr_reflect_block_kernel(QrArgs a) {
  __shared__ double sTV[NB * (NB + 1)];                  // the prologue's T, as the vector kernel lays it out; then the chunk of V_p [c][row]
  __shared__ double sd[KB][NB], sw[NB][KB], spart[KB][4][NB], sz[KB][NB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);      // the same in a whole wave: column and right-hand-side indices stay scalar
  const int q = wv & 3, j0 = (wv >> 2) * 2;
  const int g = blockIdx.x, G = gridDim.x, kb = a.kb;
  const T *W = (const T *)a.W;
  const int64_t slots = (int64_t)QG * NB;
  if (a.jbp) {
    for (int e = tid; e < NB2; e += QBT) sTV[(e >> 6) * (NB + 1) + (e & 63)] = a.tp[e];      // T[i, l] at sTV[l * (NB + 1) + i]
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
      if (j0 + jj < kb) spart[j0 + jj][q][lane] = qr_quarter(a.pin + (j0 + jj) * slots, G, lane, q);
    __syncthreads();
    if (wv < kb) sd[wv][lane] = (spart[wv][0][lane] + spart[wv][1][lane]) + (spart[wv][2][lane] + spart[wv][3][lane]);
    __syncthreads();
    double part[2] = {0.0, 0.0};
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int l = q * 16 + t;
      const double tv = a.tp_trans ? sTV[lane * (NB + 1) + l] : sTV[l * (NB + 1) + lane];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
        if (j0 + jj < kb) part[jj] = fma(tv, sd[j0 + jj][l], part[jj]);
    }
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
      if (j0 + jj < kb) spart[j0 + jj][q][lane] = part[jj];
    __syncthreads();
    if (wv < kb) sw[lane][wv] = (spart[wv][0][lane] + spart[wv][1][lane]) + (spart[wv][2][lane] + spart[wv][3][lane]);
    __syncthreads();                                     // sTV is free for the chunks from here
  }
  double acc[4][KB];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int j = 0; j < KB; ++j) acc[u][j] = 0.0;
  const int64_t nch = (a.mf + NB - 1) / NB;
  for (int64_t ch = g; ch < nch; ch += G) {
    const int64_t r = ch * NB + lane;
    const bool in = r < a.mf;
    double zr = 0.0;
    if (wv < kb && in) {
      if (a.load == 1) zr = (double)((const T *)a.v)[(IDX ? (int64_t)a.idx[r] : r) + wv * a.ldv];
      else if (a.load == 2) zr = r < a.nf ? a.zc[r + wv * a.nf] : 0.0;
      else zr = a.z[r + wv * a.mf];
    }
    double vn[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = wv * 4 + u;
      const int64_t col = a.jn + c;
      vn[u] = (c < a.jbn && in && r > col) ? ld_stream(W + r + col * a.ld) : 1.0;
    }
    if (a.jbp) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = wv * 4 + u;
        const int64_t col = a.jp + c;
        sTV[c * NB + lane] = (c < a.jbp && in && r > col) ? ld_stream(W + r + col * a.ld) : 1.0;
      }
      __syncthreads();
      double part[2] = {0.0, 0.0};
#pragma unroll 4
      for (int t = 0; t < 16; ++t) {
        const int c = q * 16 + t;
        if (c < a.jbp && in && r >= a.jp + c) {
          const double pv = sTV[c * NB + lane];
#pragma unroll
          for (int jj = 0; jj < 2; ++jj)
            if (j0 + jj < kb) part[jj] = fma(pv, sw[c][j0 + jj], part[jj]);
        }
      }
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
        if (j0 + jj < kb) spart[j0 + jj][q][lane] = part[jj];
      __syncthreads();
      if (wv < kb) zr -= (spart[wv][0][lane] + spart[wv][1][lane]) + (spart[wv][2][lane] + spart[wv][3][lane]);
    }
    if (wv < kb) {
      if (in) {
        if (a.epi) store_res<T, BETA0>((T *)a.res + wv * a.ldr, IDX ? (int64_t)a.idx[r] : r, zr, a.alpha, a.beta);
        else if (!a.zc_out) a.z[r + wv * a.mf] = zr;
        else if (r < a.nf) a.zc[r + wv * a.nf] = zr;
      }
      if (a.jbn) sz[wv][lane] = zr;
    }
    if (a.jbn) {
      __syncthreads();
      bool on[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) on[u] = wv * 4 + u < a.jbn && in && r >= a.jn + wv * 4 + u;
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        if (j < kb) {
          const double zj = sz[j][lane];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (on[u]) acc[u][j] = fma(vn[u], zj, acc[u][j]);
        }
      }
      if (!a.jbp) __syncthreads();                       // a chain's first launch: nothing else separates these reads of sz from the next chunk
    }
  }
  if (a.jbn) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < KB; ++j)
        if (j < kb) {
          const double s = wave_sum(acc[u][j]);
          if (lane == 0) a.pout[j * slots + (int64_t)g * NB + wv * 4 + u] = s;
        }
  }
  if (a.fill_idx)
    for (int64_t i = a.fill_lo + (int64_t)g * QBT + tid; i < a.fill_hi; i += (int64_t)G * QBT) {
      const int64_t o = a.fill_idx[i];
      for (int j = 0; j < kb; ++j) store_res<T, BETA0>((T *)a.res + j * a.ldr, o, 0.0, a.alpha, a.beta);
    }
}

template <typename T>
int32_t launch_reflect_block(mxlo_ctx *ctx, const QrArgs &a) {
  const unsigned G = (unsigned)qr_grid(a.mf);
  if (a.idx) {
    if (a.beta == 0.0) hipLaunchKernelGGL((qr_reflect_block_kernel<T, true, true>), dim3(G), dim3(QBT), 0, ctx->stream, a);
    else hipLaunchKernelGGL((qr_reflect_block_kernel<T, false, true>), dim3(G), dim3(QBT), 0, ctx->stream, a);
  } else if (a.beta == 0.0) hipLaunchKernelGGL((qr_reflect_block_kernel<T, true, false>), dim3(G), dim3(QBT), 0, ctx->stream, a);
  else hipLaunchKernelGGL((qr_reflect_block_kernel<T, false, false>), dim3(G), dim3(QBT), 0, ctx->stream, a);
  MXLO_LAUNCH_CHECK();
  return MXLO_OK;
}

// doubles of work: the vector apply's, and the block apply's — z (mf x KB), two sets of QG x NB slots per right-hand side, and
// the compact nf x KB matrix the block sweep works on (it addresses its matrix with column stride n = nf)
inline int64_t qr_work(int64_t mf) { return mf + 2 * (int64_t)QG * NB; }
inline int64_t qr_block_work(int64_t mf, int64_t nf) { return KB * (mf + nf + 2 * (int64_t)QG * NB); }

// One reflector chain, nb + 1 launches over the leading nc columns of a factor with `rows` rows; launch i reads the slots
// pb[(i + 1) & 1] and leaves the slots pb[i & 1]. a carries what the stages of an apply share (z, res, alpha, beta, the group,
// zc) and is this chain's own copy. !trans: Q', blocks ascending — launch 0 loads v (through idx if given), the last launch
// of a group (a.kb > 0) writes rows < nc to zc and, given a fill, the zeros of a rank-deficient solution. trans: Q, blocks
// descending — launch 0 takes rows < nc from z (zc) and zero below, the last launch writes res (through idx if given).
struct Fill {
  const int *idx;
  int64_t lo, hi;
};

template <typename T>
int32_t reflect_chain(mxlo_ctx *ctx, QrArgs a, const T *W, int64_t ld, int64_t rows, int64_t nc, const double *tfac, double *const *pb,
                      bool trans, const T *v, const int *idx = nullptr, const Fill *fill = nullptr) {
  const int64_t nb = (nc + NB - 1) / NB;
  a.W = W; a.ld = ld; a.mf = rows; a.nf = nc; a.tp_trans = trans ? 0 : 1;
  for (int64_t i = 0; i <= nb; ++i) {
    const int64_t kp = trans ? nb - i : i - 1, kn = trans ? nb - 1 - i : i;
    a.v = (!trans && i == 0) ? v : nullptr;
    a.load = i == 0 ? (trans ? 2 : 1) : 0;
    a.jbp = a.jbn = 0;
    if (i > 0) { a.jp = kp * NB; a.jbp = (int)(nc - a.jp < NB ? nc - a.jp : NB); a.tp = tfac + kp * NB2; }
    if (i < nb) { a.jn = kn * NB; a.jbn = (int)(nc - a.jn < NB ? nc - a.jn : NB); }
    a.pin = pb[(i + 1) & 1]; a.pout = pb[i & 1];
    a.epi = trans && i == nb;
    a.zc_out = a.kb > 0 && !trans && i == nb;
    a.idx = ((!trans && i == 0) || a.epi) ? idx : nullptr;
    if (fill && !trans && i == nb) { a.fill_idx = fill->idx; a.fill_lo = fill->lo; a.fill_hi = fill->hi; }   // the last launch: none follows
    MXLO_TRY(a.kb > 0 ? launch_reflect_block<T>(ctx, a) : launch_reflect<T>(ctx, a));
  }
  return MXLO_OK;
}

// what the stages of an apply share, on the vector apply's work (ap.z; grp.kb == 0: z (mf), then two sets of QG x NB slots) or
// the block apply's (z (mf x KB), two sets of slots per right-hand side, then zc); sw is the apply as the sweep with R sees it,
// on the matrix it works on
template <typename T>
struct QrStages {
  QrArgs a{};
  double *pb[2];
  Apply<T> sw;
  QrStages(const Apply<T> &ap, int64_t mf) : sw(ap) {
    const bool blk = ap.grp.kb > 0;
    const int64_t slots = (int64_t)(blk ? KB : 1) * QG * NB, zlen = (blk ? KB : 1) * mf;
    pb[0] = ap.z + zlen; pb[1] = ap.z + zlen + slots;
    a.z = ap.z; a.res = ap.res; a.alpha = ap.alpha; a.beta = ap.beta;
    a.kb = ap.grp.kb; a.ldr = ap.grp.ldr; a.ldv = ap.grp.ldv; a.zc = blk ? pb[1] + slots : nullptr;
    sw.z = blk ? a.zc : ap.z;
  }
};

// N: x = inv(R) (Q' v)[0:nf] — the chain with Q', then the descending sweep with R, which carries the epilogue. T: y = Q [inv(R') u;
// 0] — the ascending sweep with R', then the chain with Q, whose last launch has the epilogue over all mf entries. 2 nb + 1
// launches either way, for a vector and for a group of grp.kb columns alike; the sweep with R keeps its own kernel and, for a
// group, its own nf x kb matrix zc. jpvt (the pivoted form): nf is the rank, nfull the number of columns.
template <typename T>
int32_t qr_mul_t(const Apply<T> &ap, const T *W, int64_t ld, int64_t mf, int64_t nf, const double *tfac, const double *dinv, const T *v,
                 bool trans, const int *jpvt, int64_t nfull) {
  const QrStages<T> s(ap, mf);
  const Tri<T> r{.Tm = W, .ld = ld, .n = nf, .upper = true, .dinv = dinv};
  const Fill fill{jpvt, nf, nfull};
  if (trans) MXLO_TRY(sweep(s.sw, r, {.trans = true, .v = v, .gather = jpvt}));
  MXLO_TRY(reflect_chain<T>(ap.ctx, s.a, W, ld, mf, nf, tfac, s.pb, trans, v, nullptr, jpvt ? &fill : nullptr));
  if (trans) return MXLO_OK;
  return sweep(s.sw, r, {.epi = true, .scatter = jpvt});
}

// ---------------------------------------------------------------------------------------------- cod / pinv_mul
// opPinv for a numerical rank r < nf: the complete orthogonal decomposition on top of geqp3's F P = Q1 [R11 R12; 0 0]. With
// S = [R11 R12]' (nf x r, full column rank) factored as S = Q2 R2 by the unpivoted chain above, [R11 R12] = R2' Q2' and
//   pinv(F) = P Q2 inv(R2') [I_r 0] Q1',    pinv(F)' = Q1 [I_r; 0] inv(R2) Q2' P'.
// An apply is two reflector chains joined by one sweep with R2: 3 ceil(r/64) + 2 launches.

// W2 = S: W2[i, c] = W[c, i] for c <= i, zero above the diagonal (where W holds reflector vectors); an NB x NB tile of W is
// read with unit stride along its rows c and written with unit stride along i, turned through LDS as qr_copy_kernel does
template <typename T>
__global__ void __launch_bounds__(kBlock) cod_extract_kernel(T *__restrict__ W2, const T *__restrict__ W, int64_t ldw, int64_t nf,
                                                             int64_t rank) {
  __shared__ T s[NB * (NB + 1)];
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * NB, c0 = (int64_t)blockIdx.y * NB;
  for (int il = q; il < NB; il += 4) {
    const int64_t i = i0 + il, c = c0 + lane;
    s[il * (NB + 1) + lane] = (i < nf && c < rank && c <= i) ? W[c + i * ldw] : T(0);
  }
  __syncthreads();
  for (int cl = q; cl < NB; cl += 4) {
    const int64_t i = i0 + lane, c = c0 + cl;
    if (i < nf && c < rank) W2[i + c * nf] = s[lane * (NB + 1) + cl];
  }
}

template <typename T>
int32_t cod_factor_t(mxlo_ctx *ctx, const T *W, int64_t ldw, int64_t nf, int64_t rank, T *W2, double *tfac2, double *dinv2,
                     double *fwork, int *info_dev) {
  MXLO_HIP(hipMemsetAsync(info_dev, 0, sizeof(int), ctx->stream));
  hipLaunchKernelGGL((cod_extract_kernel<T>), dim3((unsigned)((nf + NB - 1) / NB), (unsigned)((rank + NB - 1) / NB)), dim3(kBlock), 0,
                     ctx->stream, W2, W, ldw, nf, rank);
  MXLO_LAUNCH_CHECK();
  return geqrf_chain_t<T>(ctx, W2, nf, nf, rank, tfac2, dinv2, fwork, info_dev);
}

// The factor of geqp3 (W, tfac; mf x nf, rank r < nf), the permutation and the second factor (W2: nf x r with ld nf, tfac2,
// dinv2). N: res (nf) — Q1' over the leading r columns of W, w = inv(R2') z[0:r], Q2 [w; 0] over the nf rows of W2 with
// res[jpvt[i]] written by the epilogue. T: res (mf) — Q2' over W2 with z[i] = u[jpvt[i]] gathered by launch 0, w = inv(R2)
// z[0:r], Q1 [w; 0]. work is qr_mul_t's, for a vector or for a group: the second chain's z has nf <= mf rows, its sweep
// matrix r <= nf, and both chains use the same two sets of slots, so nothing more is needed.
template <typename T>
int32_t pinv_mul_t(const Apply<T> &ap, const T *W, int64_t ld, int64_t mf, int64_t nf, const double *tfac, const int *jpvt, int64_t r,
                   const T *W2, const double *tfac2, const double *dinv2, const T *v, bool trans) {
  mxlo_ctx *ctx = ap.ctx;
  const QrStages<T> s(ap, mf);
  if (!trans) MXLO_TRY(reflect_chain<T>(ctx, s.a, W, ld, mf, r, tfac, s.pb, false, v));
  else MXLO_TRY(reflect_chain<T>(ctx, s.a, W2, nf, nf, r, tfac2, s.pb, false, v, jpvt));
  MXLO_TRY(sweep(s.sw, {.Tm = W2, .ld = nf, .n = r, .upper = true, .dinv = dinv2}, {.trans = !trans}));
  if (!trans) return reflect_chain<T>(ctx, s.a, W2, nf, nf, r, tfac2, s.pb, true, (const T *)nullptr, jpvt);
  return reflect_chain<T>(ctx, s.a, W, ld, mf, r, tfac, s.pb, true, (const T *)nullptr);
}

// ---------------------------------------------------------------------------------------------- geqp3
// F P = Q R with column pivoting, right-looking, ONE column per step, three launches per step (below). The grids of a step are
// 2-D — row groups x tiles of NB trailing columns — so a workgroup adds up only its own tile's partial sums. The chunks of NB
// rows from the diagonal's chunk down are dealt round-robin to at most QPG row groups; tiles and chunks are aligned to NB in
// absolute indices. A step reads the two columns it exchanges only through copies (xbuf: the pivot column, cbuf: the one it
// displaces) that the launch before made, so no workgroup reads what another one of the same launch writes. The squared
// norms of the trailing columns are RECOMPUTED by the pass that has just written them, never downdated.
constexpr int QPG = 64;              // most row groups of a step = partial slots per column

struct QpScratch {
  double *npart, *dpart, *sig, *drow, *taus, *xbuf, *cbuf, *gpart;
  int *piv;
};

inline int64_t geqp3_scratch(int64_t mf, int64_t nf) { return 2 * (int64_t)QPG * nf + QPG + 2 * nf + 2 * mf + 2 + (int64_t)QPG * NB2; }

inline QpScratch qp_layout(double *s, int64_t mf, int64_t nf) {
  QpScratch l;
  l.npart = s; s += (int64_t)QPG * nf;
  l.dpart = s; s += (int64_t)QPG * nf;
  l.sig = s; s += QPG;
  l.drow = s; s += nf;
  l.taus = s; s += nf;
  l.xbuf = s; s += mf;
  l.cbuf = s; s += mf;
  l.piv = (int *)s; s += 2;
  l.gpart = s;
  return l;
}

// step 1, one workgroup: the squared norms of the columns c .. nf - 1 over the rows from c down, each the sum of the Gp partial
// sums the launch before left, in order; the first largest one is the pivot: piv[0] = its column, jpvt[c] <-> jpvt[piv]. A norm
// that is not finite (NaN counts as the largest), or a largest norm of zero at c == 0, stores c + 1 in *info.
__global__ void __launch_bounds__(kBlock) geqp3_pivot_kernel(const double *__restrict__ npart, int Gp, int64_t nf, int64_t c, int *jpvt,
                                                             int *piv, int *info) {
  __shared__ double sv[kBlock];
  __shared__ int sj[kBlock], sbad;
  if (*info != 0) return;
  const int tid = threadIdx.x;
  if (tid == 0) sbad = 0;
  if (c == 0)
    for (int64_t j = tid; j < nf; j += kBlock) jpvt[j] = (int)j;
  __syncthreads();
  double best = -1.0;
  int bj = 0x7fffffff;
  for (int64_t j = c + tid; j < nf; j += kBlock) {
    double s = 0.0;
    for (int g = 0; g < Gp; ++g) s += npart[(int64_t)g * nf + j];
    if (!(s < __builtin_inf())) sbad = 1;
    if (s > best) { best = s; bj = (int)j; }
  }
  sv[tid] = best; sj[tid] = bj;
  __syncthreads();
  for (int h = kBlock / 2; h > 0; h >>= 1) {
    if (tid < h) {
      const double o = sv[tid + h];
      const int oj = sj[tid + h];
      if (o > sv[tid] || (o == sv[tid] && oj < sj[tid])) { sv[tid] = o; sj[tid] = oj; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (sbad || (c == 0 && sv[0] == 0.0)) *info = (int)(c + 1);
    else {
      const int p = sj[0], t = jpvt[c];
      piv[0] = p;
      jpvt[c] = jpvt[p]; jpvt[p] = t;
    }
  }
}

// step 2, grid (row groups, tiles): x = the pivot column (memory column p), which becomes column c. Leaves the partial dots
// of x below row c with every trailing column of the tile (memory column c standing in for column p), row c of those columns
// (drow), and — tile 0 — the partial sums of sigma = |x below row c|^2 and the copies xbuf / cbuf of the memory columns p / c
// over their whole height. Nothing of W is written.
template <typename T>
__global__ void __launch_bounds__(kBlock) geqp3_dot_kernel(const T *__restrict__ W, int64_t ld, int64_t mf, int64_t nf, int64_t c,
                                                           const int *__restrict__ piv, double *__restrict__ dpart,
                                                           double *__restrict__ sig, double *__restrict__ drow,
                                                           double *__restrict__ xbuf, double *__restrict__ cbuf, const int *info) {
  if (*info != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int g = blockIdx.x, G = gridDim.x;
  const bool t0 = blockIdx.y == 0;
  const int64_t p = piv[0];
  const int64_t ch0 = c / NB, nch = (mf + NB - 1) / NB, tlo = ((c + 1) / NB + blockIdx.y) * NB;
  const T *xc = W + p * ld, *oc = W + c * ld;
  double acc[16], sacc = 0.0;
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = 0.0;
  for (int64_t ch = ch0 + g; ch < nch; ch += G) {
    const int64_t r = ch * NB + lane;
    const bool in = r < mf;
    const double xr = in ? (double)xc[r] : 0.0, xd = r > c ? xr : 0.0;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int64_t j = tlo + q * 16 + t;
      if (in && j > c && j < nf) {
        const double val = (double)(j == p ? oc[r] : W[r + j * ld]);
        acc[t] = fma(val, xd, acc[t]);
        if (r == c) drow[j] = val;
      }
    }
    if (t0 && q == 0 && in) {
      xbuf[r] = xr;
      cbuf[r] = (double)oc[r];
      sacc = fma(xd, xd, sacc);
    }
  }
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int64_t j = tlo + q * 16 + t;
    const double s = wave_sum(acc[t]);
    if (lane == 0 && j > c && j < nf) dpart[(int64_t)g * nf + j] = s;
  }
  if (t0 && q == 0) {
    const double s = wave_sum(sacc);
    if (lane == 0) sig[g] = s;
  }
  if (t0 && g == 0)
    for (int64_t r = tid; r < ch0 * NB; r += kBlock) { xbuf[r] = (double)xc[r]; cbuf[r] = (double)oc[r]; }
}

// step 3, the same grid: adds up its tile's dots and sigma, forms the reflector of column c exactly as geqrf_panel_kernel does
// (larfg: beta = -sign(alpha) |(alpha, x)|, tau = (beta - alpha) / beta, v = x / (alpha - beta); x == 0: tau = 0, H = I),
// applies it to its rows of the tile's trailing columns — column p takes the displaced column from cbuf, over its whole
// height — and leaves the partial squared norms of what it wrote below row c for the next step 1. Tile 0 writes column c:
// R above the diagonal, beta on it, v below. c == -1: only the norms, of all columns over all rows. A norm that is not finite
// stores c + 1 in *info; a zero one is a legitimate rank-deficient step.
template <typename T>
__global__ void __launch_bounds__(kBlock) geqp3_reflect_kernel(T *W, int64_t ld, int64_t mf, int64_t nf, int64_t c,
                                                               const int *__restrict__ piv, const double *__restrict__ dpart,
                                                               const double *__restrict__ sig, const double *__restrict__ drow,
                                                               const double *__restrict__ xbuf, const double *__restrict__ cbuf,
                                                               double *__restrict__ taus, double *__restrict__ npart, int *info) {
  __shared__ double sW[NB], spart[4][NB];
  if (*info != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int g = blockIdx.x, G = gridDim.x;
  const bool t0 = blockIdx.y == 0;
  const int64_t p = c >= 0 ? (int64_t)piv[0] : -1;
  const int64_t ch0 = (c < 0 ? 0 : c) / NB, nch = (mf + NB - 1) / NB, tlo = ((c + 1) / NB + blockIdx.y) * NB;
  double scale = 0.0, beta = 0.0;
  if (c >= 0) {
    const int64_t jl = tlo + lane;
    double a = 0.0;
    if (jl > c && jl < nf)
      for (int gg = q; gg < G; gg += 4) a += dpart[(int64_t)gg * nf + jl];
    spart[q][lane] = a;
    double sigma = 0.0;
    for (int gg = 0; gg < G; ++gg) sigma += sig[gg];
    __syncthreads();
    const double alpha = xbuf[c];
    const double nrm = sqrt(fma(alpha, alpha, sigma));
    if (!(nrm < __builtin_inf())) {                      // the same value in every thread of every workgroup
      if (g == 0 && t0 && tid == 0) *info = (int)(c + 1);
      return;
    }
    double tau = 0.0;
    beta = alpha;
    if (sigma != 0.0) {
      beta = -copysign(nrm, alpha);
      tau = (beta - alpha) / beta;
      scale = 1.0 / (alpha - beta);
    }
    if (tid < NB) {
      const int64_t j = tlo + tid;
      const double dot = (spart[0][tid] + spart[1][tid]) + (spart[2][tid] + spart[3][tid]);
      sW[tid] = (j > c && j < nf) ? tau * fma(scale, dot, drow[j]) : 0.0;
    }
    if (g == 0 && t0 && tid == 0) taus[c] = tau;
    __syncthreads();
  }
  double acc[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = 0.0;
  for (int64_t ch = ch0 + g; ch < nch; ch += G) {
    const int64_t r = ch * NB + lane;
    const bool in = r < mf;
    double vr = 0.0;
    if (c >= 0 && in) vr = r > c ? (double)(T)(xbuf[r] * scale) : (r == c ? 1.0 : 0.0);
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int64_t j = tlo + q * 16 + t;
      if (in && j > c && j < nf) {
        const double val = j == p ? cbuf[r] : (double)W[r + j * ld];
        T x = (T)val;
        if (c >= 0) {
          if (r >= c) x = (T)fma(-sW[q * 16 + t], vr, val);
          if (r >= c || j == p) W[r + j * ld] = x;
        }
        if (r > c) acc[t] = fma((double)x, (double)x, acc[t]);
      }
    }
    if (c >= 0 && t0 && q == 0 && in) W[r + c * ld] = r > c ? (T)vr : (r == c ? (T)beta : (T)xbuf[r]);
  }
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int64_t j = tlo + q * 16 + t;
    const double s = wave_sum(acc[t]);
    if (lane == 0 && j > c && j < nf) npart[(int64_t)g * nf + j] = s;
  }
  if (c >= 0 && t0 && g == 0)                            // the rows of R above the diagonal's chunk
    for (int64_t r = tid; r < ch0 * NB; r += kBlock) {
      W[r + c * ld] = (T)xbuf[r];
      if (p != c) W[r + p * ld] = (T)cbuf[r];
    }
}

// after the last step, one workgroup: rank = the length of the leading run of j with |R_jj| > rtol |R_00|, into info[1]
template <typename T>
__global__ void __launch_bounds__(kBlock) geqp3_rank_kernel(const T *__restrict__ W, int64_t ld, int64_t nf, double rtol, int *info) {
  __shared__ int sm[kBlock];
  const int tid = threadIdx.x;
  if (info[0] != 0) return;
  const double thr = rtol * fabs((double)W[0]);
  int first = (int)nf;
  for (int64_t j = tid; j < nf; j += kBlock)
    if (!(fabs((double)W[j + j * ld]) > thr)) { first = (int)j; break; }
  sm[tid] = first;
  __syncthreads();
  for (int h = kBlock / 2; h > 0; h >>= 1) {
    if (tid < h && sm[tid + h] < sm[tid]) sm[tid] = sm[tid + h];
    __syncthreads();
  }
  if (tid == 0) info[1] = sm[0];
}

// larft for one block column (columns j0 .. j0 + jb of the factor, rows from j0 down), two launches. (1) The partial Gram
// matrices V' V of the panel, V with its implicit unit diagonal, one per row group, the chunks of a group in order.
template <typename T>
__global__ void __launch_bounds__(kBlock) geqp3_gram_kernel(const T *__restrict__ W, int64_t ld, int64_t mf, int64_t j0, int jb,
                                                            double *__restrict__ gpart) {
  __shared__ double sV[NB][NB + 1];                      // [column][row of the chunk]
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int g = blockIdx.x, G = gridDim.x;
  const int64_t nch = (mf - j0 + NB - 1) / NB;
  double acc[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = 0.0;
  for (int64_t ch = g; ch < nch; ch += G) {
    const int64_t r = j0 + ch * NB + lane;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int col = q * 16 + t;
      const int64_t d = j0 + col;
      double v = 0.0;
      if (col < jb && r < mf) v = r > d ? (double)W[r + d * ld] : (r == d ? 1.0 : 0.0);
      sV[col][lane] = v;
    }
    __syncthreads();
    for (int row = 0; row < NB; ++row) {
      const double a = sV[lane][row];
#pragma unroll
      for (int t = 0; t < 16; ++t) acc[t] = fma(a, sV[q * 16 + t][row], acc[t]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < 16; ++t) gpart[(int64_t)g * NB2 + lane + (q * 16 + t) * NB] = acc[t];
}

// (2) one workgroup: column c of T from column c of the Gram matrix (the G partial ones added in four strided quarters, then
// (p0 + p1) + (p2 + p3)): T[0:c, c] = -tau_c T[0:c, 0:c] (V[:, 0:c]' v_c), T[c, c] = tau_c, as geqrf_panel_kernel builds it;
// the rest of the 64 x 64 block is zero.
__global__ void __launch_bounds__(kBlock) geqp3_larft_kernel(const double *__restrict__ gpart, int G, const double *__restrict__ taus,
                                                             int jb, double *__restrict__ tf) {
  __shared__ double sT[NB2], sg[NB], spart[4][NB];
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  for (int e = tid; e < NB2; e += kBlock) sT[e] = 0.0;
  __syncthreads();
  for (int c = 0; c < jb; ++c) {
    double a = 0.0;
    for (int gg = q; gg < G; gg += 4) a += gpart[(int64_t)gg * NB2 + lane + c * NB];
    spart[q][lane] = a;
    __syncthreads();
    if (q == 0) sg[lane] = (spart[0][lane] + spart[1][lane]) + (spart[2][lane] + spart[3][lane]);
    __syncthreads();
    if (tid < NB) {
      const double tau = taus[c];
      double t = 0.0;
      if (tid < c) {
        for (int l = tid; l < c; ++l) t = fma(sT[tid + l * NB], sg[l], t);
        t = -tau * t;
      } else if (tid == c) t = tau;
      sT[tid + c * NB] = t;
    }
    __syncthreads();
  }
  for (int e = tid; e < NB2; e += kBlock) tf[e] = sT[e];
}

// the chain up to the rank: 3 nf + 3 launches whose grids depend on (mf, nf) only; info_dev[0] = info, info_dev[1] = rank
template <typename T>
int32_t geqp3_t(mxlo_ctx *ctx, const T *M, int64_t ldm, int trans, T *W, int64_t ldw, int64_t mf, int64_t nf, int *jpvt, double rtol,
                const QpScratch &l, int *info_dev) {
  const int64_t nbt = (nf + NB - 1) / NB, nch = (mf + NB - 1) / NB;
  MXLO_HIP(hipMemsetAsync(info_dev, 0, 2 * sizeof(int), ctx->stream));
  hipLaunchKernelGGL((qr_copy_kernel<T>), dim3((unsigned)nch, (unsigned)nbt), dim3(kBlock), 0, ctx->stream, W, ldw, M, ldm, trans, mf, nf);
  MXLO_LAUNCH_CHECK();
  int Gp = (int)(nch < QPG ? nch : QPG);
  hipLaunchKernelGGL((geqp3_reflect_kernel<T>), dim3((unsigned)Gp, (unsigned)nbt), dim3(kBlock), 0, ctx->stream, W, ldw, mf, nf,
                     (int64_t)-1, (const int *)l.piv, (const double *)l.dpart, (const double *)l.sig, (const double *)l.drow,
                     (const double *)l.xbuf, (const double *)l.cbuf, l.taus, l.npart, info_dev);
  MXLO_LAUNCH_CHECK();
  for (int64_t c = 0; c < nf; ++c) {
    hipLaunchKernelGGL(geqp3_pivot_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, (const double *)l.npart, Gp, nf, c, jpvt, l.piv, info_dev);
    MXLO_LAUNCH_CHECK();
    const int64_t rch = nch - c / NB, tl = nbt - (c + 1) / NB;
    const dim3 grid((unsigned)(rch < QPG ? rch : QPG), (unsigned)(tl < 1 ? 1 : tl));
    hipLaunchKernelGGL((geqp3_dot_kernel<T>), grid, dim3(kBlock), 0, ctx->stream, (const T *)W, ldw, mf, nf, c, (const int *)l.piv, l.dpart,
                       l.sig, l.drow, l.xbuf, l.cbuf, (const int *)info_dev);
    MXLO_LAUNCH_CHECK();
    hipLaunchKernelGGL((geqp3_reflect_kernel<T>), grid, dim3(kBlock), 0, ctx->stream, W, ldw, mf, nf, c, (const int *)l.piv,
                       (const double *)l.dpart, (const double *)l.sig, (const double *)l.drow, (const double *)l.xbuf,
                       (const double *)l.cbuf, l.taus, l.npart, info_dev);
    MXLO_LAUNCH_CHECK();
    Gp = (int)grid.x;
  }
  hipLaunchKernelGGL((geqp3_rank_kernel<T>), dim3(1), dim3(kBlock), 0, ctx->stream, (const T *)W, ldw, nf, rtol, info_dev);
  MXLO_LAUNCH_CHECK();
  return MXLO_OK;
}

// once the rank is known: T of the leading rank columns, block column by block column, and the block inverses of R11
template <typename T>
int32_t geqp3_finish_t(mxlo_ctx *ctx, const T *W, int64_t ldw, int64_t mf, int64_t rank, double *tfac, double *dinv, const QpScratch &l) {
  const int64_t nb = (rank + NB - 1) / NB;
  for (int64_t k = 0; k < nb; ++k) {
    const int64_t j0 = k * NB, jb = rank - j0 < NB ? rank - j0 : NB, rch = (mf - j0 + NB - 1) / NB;
    const int G = (int)(rch < QPG ? rch : QPG);
    hipLaunchKernelGGL((geqp3_gram_kernel<T>), dim3((unsigned)G), dim3(kBlock), 0, ctx->stream, W, ldw, mf, j0, (int)jb, l.gpart);
    MXLO_LAUNCH_CHECK();
    hipLaunchKernelGGL(geqp3_larft_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, (const double *)l.gpart, G, (const double *)(l.taus + j0),
                       (int)jb, tfac + k * NB2);
    MXLO_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL((tri_prepare_kernel<T>), dim3((unsigned)nb), dim3(kBlock), 0, ctx->stream, W, ldw, rank, 1, dinv);
  MXLO_LAUNCH_CHECK();
  return MXLO_OK;
}

}  // namespace

namespace {
// the tall orientation every entry point of the rectangular family takes, 1 <= nf <= mf <= ldw, within the index range of the
// kernels; grid_limit: a factorisation also has the block columns in a grid dimension
int32_t check_tall(int64_t mf, int64_t nf, int64_t ldw, bool grid_limit, const char *what) {
  MXLO_REQUIRE(nf >= 1 && mf >= nf && ldw >= mf, MXLO_ESHAPE, "%s: mf = %lld, nf = %lld (1 <= nf <= mf), ldw = %lld", what, (long long)mf,
               (long long)nf, (long long)ldw);
  MXLO_REQUIRE(mf < (1LL << 31) - NB && (!grid_limit || (nf + NB - 1) / NB <= 65535), MXLO_ESHAPE, "%s: mf = %lld, nf = %lld is too large",
               what, (long long)mf, (long long)nf);
  return MXLO_OK;
}

int32_t check_scratch(int64_t scratch_len, int64_t needed, const char *what) {
  MXLO_REQUIRE(scratch_len >= needed, MXLO_ESHAPE, "%s: scratch of %lld doubles, %lld needed", what, (long long)scratch_len, (long long)needed);
  return MXLO_OK;
}

// M as mxlo_geqrf and mxlo_geqp3 find it stored: mr x mc, column-major (m_trans: the nf x mf storage of F')
int32_t check_source(const void *M, int64_t ldm, int32_t m_trans, int64_t mf, int64_t nf, int64_t es, Buf &m, const char *what) {
  const int64_t mr = m_trans ? nf : mf, mc = m_trans ? mf : nf;
  MXLO_REQUIRE(ldm >= mr, MXLO_ESHAPE, "%s: ldm = %lld < %lld", what, (long long)ldm, (long long)mr);
  m = {M, mat_bytes(mr, mc, ldm, es), "M"};
  return MXLO_OK;
}

// What the six rectangular applies check first: ctx, dtype, op_mode, the shape and — rank_max >= 0: the pivoted forms — the
// rank. Sizes that feed a byte extent are computed after this, from a valid shape. A vector entry point then passes
// k = 1 in the leading dimension mf, which holds either operand.
int32_t check_qr_shape(mxlo_ctx *ctx, int32_t dtype, int32_t op_mode, int64_t ldw, int64_t mf, int64_t nf, int64_t rank, int64_t rank_max,
                       const char *what) {
  MXLO_TRY(check_real(ctx, dtype, what));
  MXLO_TRY(check_mode(op_mode, what));
  MXLO_TRY(check_tall(mf, nf, ldw, false, what));
  MXLO_REQUIRE(rank_max < 0 || (rank >= 1 && rank <= rank_max), MXLO_ESHAPE, "%s: rank = %lld (1 <= rank <= %lld for nf = %lld)", what,
               (long long)rank, (long long)rank_max, (long long)nf);
  return MXLO_OK;
}

// res and V of a rectangular apply: columns() with the rows op_mode gives them. A vector entry point passes qr_vectors(): k = 1 in the
// leading dimension mf, which holds either operand.
inline Operands qr_operands(const void *res, int64_t ldr, const void *V, int64_t ldv, int64_t k, int64_t mf, int64_t nf, int32_t op_mode) {
  const bool tr = op_mode != MXLO_OP_N;
  return columns(res, ldr, V, ldv, k, tr ? mf : nf, tr ? nf : mf);
}
inline Operands qr_vectors(const void *res, const void *v, int64_t mf, int64_t nf, int32_t op_mode) {
  Operands o = qr_operands(res, mf, v, mf, 1, mf, nf, op_mode);
  o.block = false;
  return o;
}

// mxlo_qr_mul* and, with jpvt and the rank, mxlo_qrp_mul*; o.block: the work space is qr_block_work's. The T factors and the
// block inverses count as those of all nf columns, whatever the rank.
int32_t check_qr_apply(mxlo_ctx *ctx, int32_t dtype, const Operands &o, const void *W, int64_t ldw, int64_t mf, int64_t nf,
                       const double *tfac, const double *dinv, bool pivoted, const int32_t *jpvt, int64_t rank, const double *work,
                       int32_t op_mode, const char *what, bool &go) {
  go = false;
  MXLO_TRY(check_qr_shape(ctx, dtype, op_mode, ldw, mf, nf, rank, pivoted ? nf : -1, what));
  MXLO_TRY(check_operands(dtype, o, false,
                          {{W, mat_bytes(mf, nf, ldw, esize(dtype)), "the factor"},
                           {tfac, blocks_bytes(nf), "the T factors"},
                           {dinv, blocks_bytes(nf), "the block inverses"},
                           {work, (o.block ? qr_block_work(mf, nf) : qr_work(mf)) * 8, "the work space"}},
                          what, go));
  return pivoted && go ? check_owned(dtype, o, {{jpvt, nf * 4, "the permutation"}}, what) : MXLO_OK;
}

// mxlo_pinv_mul*: rank < nf (rank == nf is mxlo_qrp_mul's), and both factors; the T factors and the block inverses of both
// count as those of `rank` columns
int32_t check_pinv(mxlo_ctx *ctx, int32_t dtype, const Operands &o, const void *W, int64_t ldw, int64_t mf, int64_t nf, const double *tfac,
                   const int32_t *jpvt, int64_t rank, const void *W2, const double *tfac2, const double *dinv2, const double *work,
                   int32_t op_mode, const char *what, bool &go) {
  go = false;
  MXLO_TRY(check_qr_shape(ctx, dtype, op_mode, ldw, mf, nf, rank, nf - 1, what));
  const int64_t es = esize(dtype);
  return check_operands(dtype, o, false,
                        {{W, mat_bytes(mf, nf, ldw, es), "the factor"},
                         {tfac, blocks_bytes(rank), "the T factors"},
                         {jpvt, nf * 4, "the permutation"},
                         {W2, nf * rank * es, "the second factor"},
                         {tfac2, blocks_bytes(rank), "the second T factors"},
                         {dinv2, blocks_bytes(rank), "the block inverses"},
                         {work, (o.block ? qr_block_work(mf, nf) : qr_work(mf)) * 8, "the work space"}},
                        what, go);
}

// the one body of mxlo_qr_mul* and, pivoted, of mxlo_qrp_mul*, where the chain takes the leading `rank` columns
int32_t qr_mul(mxlo_ctx *ctx, int32_t dtype, const Operands &o, const void *W, int64_t ldw, int64_t mf, int64_t nf, const double *tfac,
               const double *dinv, bool pivoted, const int32_t *jpvt, int64_t rank, double *work, int32_t op_mode, double alpha,
               double beta, const char *what) {
  bool go;
  MXLO_TRY(check_qr_apply(ctx, dtype, o, W, ldw, mf, nf, tfac, dinv, pivoted, jpvt, rank, work, op_mode, what, go));
  if (!go) return MXLO_OK;
  MXLO_DEVICE_GUARD(ctx);
  const bool tr = op_mode != MXLO_OP_N;
  return for_real_groups(dtype, o, [&]<typename T>(T *r, const T *v, Group grp) {
    return qr_mul_t<T>({ctx, r, alpha, beta, work, grp}, (const T *)W, ldw, mf, pivoted ? rank : nf, tfac, dinv, v, tr,
                       pivoted ? jpvt : nullptr, nf);
  });
}

int32_t pinv_mul(mxlo_ctx *ctx, int32_t dtype, const Operands &o, const void *W, int64_t ldw, int64_t mf, int64_t nf, const double *tfac,
                 const int32_t *jpvt, int64_t rank, const void *W2, const double *tfac2, const double *dinv2, double *work,
                 int32_t op_mode, double alpha, double beta, const char *what) {
  bool go;
  MXLO_TRY(check_pinv(ctx, dtype, o, W, ldw, mf, nf, tfac, jpvt, rank, W2, tfac2, dinv2, work, op_mode, what, go));
  if (!go) return MXLO_OK;
  MXLO_DEVICE_GUARD(ctx);
  const bool tr = op_mode != MXLO_OP_N;
  return for_real_groups(dtype, o, [&]<typename T>(T *r, const T *v, Group grp) {
    return pinv_mul_t<T>({ctx, r, alpha, beta, work, grp}, (const T *)W, ldw, mf, nf, tfac, jpvt, rank, (const T *)W2, tfac2, dinv2, v, tr);
  });
}
}  // namespace

MXLO_API int32_t mxlo_geqrf(mxlo_ctx *ctx, int32_t dtype, const void *M, int64_t ldm, int32_t m_trans, void *W, int64_t ldw, int64_t mf,
                            int64_t nf, double *tfac, double *dinv, double *scratch, int64_t scratch_len, int32_t *info_dev,
                            int32_t *info) {
  const char *what = "mxlo_geqrf";
  MXLO_TRY(check_real(ctx, dtype, what));
  MXLO_TRY(check_tall(mf, nf, ldw, true, what));
  MXLO_REQUIRE(M && W && tfac && dinv && scratch && info_dev && info, MXLO_EINVAL, "%s: null operand", what);
  *info = 0;
  const int64_t es = esize(dtype);
  Buf m;
  MXLO_TRY(check_source(M, ldm, m_trans, mf, nf, es, m, what));
  MXLO_TRY(check_scratch(scratch_len, geqrf_scratch(nf), what));
  MXLO_TRY(disjoint({m, {W, mat_bytes(mf, nf, ldw, es), "the factor"}, {tfac, blocks_bytes(nf), "the T factors"},
                     {dinv, blocks_bytes(nf), "the block inverses"}, {scratch, scratch_len * 8, "the scratch"}, {info_dev, 4, "the info word"}},
                    what));
  MXLO_TRY(refuse_capture(ctx, what));
  MXLO_DEVICE_GUARD(ctx);
  MXLO_TRY(with_real(dtype, [&]<typename T>() {
    return geqrf_t<T>(ctx, (const T *)M, ldm, m_trans ? 1 : 0, (T *)W, ldw, mf, nf, tfac, dinv, scratch, info_dev);
  }));
  return read_back(ctx, info_dev, info, 1);
}

MXLO_API int32_t mxlo_qr_mul(mxlo_ctx *ctx, int32_t dtype, void *res, const void *W, int64_t ldw, int64_t mf, int64_t nf,
                             const double *tfac, const double *dinv, double *work, const void *v, int32_t op_mode, double alpha,
                             double beta) {
  return qr_mul(ctx, dtype, qr_vectors(res, v, mf, nf, op_mode), W, ldw, mf, nf, tfac, dinv, false, nullptr, 0, work, op_mode, alpha, beta,
                "mxlo_qr_mul");
}

MXLO_API int32_t mxlo_qr_mul_block(mxlo_ctx *ctx, int32_t dtype, void *res, int64_t ldr, const void *W, int64_t ldw, int64_t mf,
                                   int64_t nf, const double *tfac, const double *dinv, double *work, const void *V, int64_t ldv,
                                   int64_t k, int32_t op_mode, double alpha, double beta) {
  return qr_mul(ctx, dtype, qr_operands(res, ldr, V, ldv, k, mf, nf, op_mode), W, ldw, mf, nf, tfac, dinv, false, nullptr, 0, work,
                op_mode, alpha, beta, "mxlo_qr_mul_block");
}

MXLO_API int32_t mxlo_geqp3(mxlo_ctx *ctx, int32_t dtype, const void *M, int64_t ldm, int32_t m_trans, void *W, int64_t ldw, int64_t mf,
                            int64_t nf, double *tfac, double *dinv, int32_t *jpvt, double rtol, double *scratch, int64_t scratch_len,
                            int32_t *info_dev, int32_t *info, int32_t *rank) {
  const char *what = "mxlo_geqp3";
  MXLO_TRY(check_real(ctx, dtype, what));
  MXLO_TRY(check_tall(mf, nf, ldw, true, what));
  MXLO_REQUIRE(rtol >= 0.0 && rtol < 1.0, MXLO_EINVAL, "%s: rtol = %g (0 <= rtol < 1)", what, rtol);
  MXLO_REQUIRE(M && W && tfac && dinv && jpvt && scratch && info_dev && info && rank, MXLO_EINVAL, "%s: null operand", what);
  *info = 0;
  *rank = 0;
  const int64_t es = esize(dtype);
  Buf m;
  MXLO_TRY(check_source(M, ldm, m_trans, mf, nf, es, m, what));
  MXLO_TRY(check_scratch(scratch_len, geqp3_scratch(mf, nf), what));
  MXLO_TRY(disjoint({m, {W, mat_bytes(mf, nf, ldw, es), "the factor"}, {tfac, blocks_bytes(nf), "the T factors"},
                     {dinv, blocks_bytes(nf), "the block inverses"}, {jpvt, nf * 4, "the permutation"},
                     {scratch, scratch_len * 8, "the scratch"}, {info_dev, 8, "the info words"}},
                    what));
  MXLO_TRY(refuse_capture(ctx, what));
  MXLO_DEVICE_GUARD(ctx);
  const QpScratch l = qp_layout(scratch, mf, nf);
  MXLO_TRY(with_real(dtype, [&]<typename T>() {
    return geqp3_t<T>(ctx, (const T *)M, ldm, m_trans ? 1 : 0, (T *)W, ldw, mf, nf, jpvt, rtol, l, info_dev);
  }));
  int32_t words[2] = {0, 0};
  MXLO_TRY(read_back(ctx, info_dev, words, 2));
  *info = words[0];
  *rank = words[1];
  if (words[0] != 0 || words[1] < 1) return MXLO_OK;
  return with_real(dtype, [&]<typename T>() { return geqp3_finish_t<T>(ctx, (const T *)W, ldw, mf, words[1], tfac, dinv, l); });
}

MXLO_API int32_t mxlo_qrp_mul(mxlo_ctx *ctx, int32_t dtype, void *res, const void *W, int64_t ldw, int64_t mf, int64_t nf,
                              const double *tfac, const double *dinv, const int32_t *jpvt, int64_t rank, double *work, const void *v,
                              int32_t op_mode, double alpha, double beta) {
  return qr_mul(ctx, dtype, qr_vectors(res, v, mf, nf, op_mode), W, ldw, mf, nf, tfac, dinv, true, jpvt, rank, work, op_mode, alpha, beta,
                "mxlo_qrp_mul");
}

MXLO_API int32_t mxlo_qrp_mul_block(mxlo_ctx *ctx, int32_t dtype, void *res, int64_t ldr, const void *W, int64_t ldw, int64_t mf,
                                    int64_t nf, const double *tfac, const double *dinv, const int32_t *jpvt, int64_t rank, double *work,
                                    const void *V, int64_t ldv, int64_t k, int32_t op_mode, double alpha, double beta) {
  return qr_mul(ctx, dtype, qr_operands(res, ldr, V, ldv, k, mf, nf, op_mode), W, ldw, mf, nf, tfac, dinv, true, jpvt, rank, work, op_mode,
                alpha, beta, "mxlo_qrp_mul_block");
}

MXLO_API int32_t mxlo_cod_factor(mxlo_ctx *ctx, int32_t dtype, const void *W, int64_t ldw, int64_t nf, int64_t rank, void *W2,
                                 double *tfac2, double *dinv2, double *scratch, int64_t scratch_len, int32_t *info_dev, int32_t *info) {
  const char *what = "mxlo_cod_factor";
  MXLO_TRY(check_real(ctx, dtype, what));
  MXLO_TRY(check_tall(nf, nf, ldw, true, what));         // of the factor's mf rows only the leading nf are read: ldw >= mf >= nf
  MXLO_REQUIRE(rank >= 1 && rank <= nf, MXLO_ESHAPE, "%s: rank = %lld (1 <= rank <= nf = %lld)", what, (long long)rank, (long long)nf);
  MXLO_REQUIRE(W && W2 && tfac2 && dinv2 && scratch && info_dev && info, MXLO_EINVAL, "%s: null operand", what);
  *info = 0;
  MXLO_TRY(check_scratch(scratch_len, geqrf_scratch(rank), what));
  const int64_t es = esize(dtype);
  MXLO_TRY(disjoint({{W, mat_bytes(rank, nf, ldw, es), "the factor"}, {W2, nf * rank * es, "the second factor"},
                     {tfac2, blocks_bytes(rank), "its T factors"}, {dinv2, blocks_bytes(rank), "its block inverses"},
                     {scratch, scratch_len * 8, "the scratch"}, {info_dev, 4, "the info word"}},
                    what));
  MXLO_TRY(refuse_capture(ctx, what));
  MXLO_DEVICE_GUARD(ctx);
  MXLO_TRY(with_real(dtype, [&]<typename T>() {
    return cod_factor_t<T>(ctx, (const T *)W, ldw, nf, rank, (T *)W2, tfac2, dinv2, scratch, info_dev);
  }));
  return read_back(ctx, info_dev, info, 1);
}

MXLO_API int32_t mxlo_pinv_mul(mxlo_ctx *ctx, int32_t dtype, void *res, const void *W, int64_t ldw, int64_t mf, int64_t nf,
                               const double *tfac, const int32_t *jpvt, int64_t rank, const void *W2, const double *tfac2,
                               const double *dinv2, double *work, const void *v, int32_t op_mode, double alpha, double beta) {
  return pinv_mul(ctx, dtype, qr_vectors(res, v, mf, nf, op_mode), W, ldw, mf, nf, tfac, jpvt, rank, W2, tfac2, dinv2, work, op_mode, alpha,
                  beta, "mxlo_pinv_mul");
}

MXLO_API int32_t mxlo_pinv_mul_block(mxlo_ctx *ctx, int32_t dtype, void *res, int64_t ldr, const void *W, int64_t ldw, int64_t mf,
                                     int64_t nf, const double *tfac, const int32_t *jpvt, int64_t rank, const void *W2,
                                     const double *tfac2, const double *dinv2, double *work, const void *V, int64_t ldv, int64_t k,
                                     int32_t op_mode, double alpha, double beta) {
  return pinv_mul(ctx, dtype, qr_operands(res, ldr, V, ldv, k, mf, nf, op_mode), W, ldw, mf, nf, tfac, jpvt, rank, W2, tfac2, dinv2, work,
                  op_mode, alpha, beta, "mxlo_pinv_mul_block");
}

// ---------------------------------------------------------------------------------------------- sytrf (Bunch-Kaufman)
// P' M P = L D L' with L unit lower triangular and D block diagonal with 1 x 1 and 2 x 2 blocks, by Bunch-Kaufman partial
// pivoting on the lower triangle, right-looking in panels. A panel is 64 or 65 columns wide: it takes columns while fewer
// than 64 are done, and a 2 x 2 pivot chosen at its 64th column takes the 65th with it. Where panel k starts is therefore
// known on the device only: starts[k], written by panel k - 1 and read by every launch of round k; the chain itself is
// ceil(n / 64) rounds whatever the data is, and a round whose start is n does nothing. Per round: (a) ONE workgroup factors the
// panel, left-looking as LAPACK's lasyf: the trailing columns of A stay as the round found them, the panel's columns are
// brought up to date one by one against the finished ones, into the n x 65 workspace Wk, which ends up holding L D beside
// the panel of L in A; (b) the panel's interchanges, in order, on the rows of every column left of it, so that L is the
// factor of the fully permuted matrix; (c) C -= L21 (L21 D)' on the lower triangle of the trailing matrix, on MFMA. One last
// launch inverts the unit lower diagonal blocks of L for the sweeps, whose blocks stay at multiples of 64.
namespace {
constexpr int SNB = NB + 1;                              // the widest panel
constexpr double BK_ALPHA = 0.6403882032022076;          // (1 + sqrt(17)) / 8

// the best (|a|, row) of the workgroup, in every thread; a thread without a candidate brings (-1, 0x7fffffff)
__device__ __forceinline__ void panel_argmax(double &best, int &bi, double *s_val, int *s_idx, int lane, int wave) {
  for (int o = 32; o; o >>= 1) {
    const double ob = __shfl_xor(best, o);
    const int oi = __shfl_xor(bi, o);
    if (pivot_better(ob, oi, best, bi)) { best = ob; bi = oi; }
  }
  if (lane == 0) { s_val[wave] = best; s_idx[wave] = bi; }
  __syncthreads();
  best = s_val[0]; bi = s_idx[0];
  for (int w = 1; w < PT / 64; ++w)
    if (pivot_better(s_val[w], s_idx[w], best, bi)) { best = s_val[w]; bi = s_idx[w]; }
  __syncthreads();
}

// wc[k .. n) = column c of the symmetric trailing matrix, brought up to date against the panel's kw finished columns:
// entry i is A[i, c] (i >= c) or A[c, i] (i < c) minus sum_j A[i, j0 + j] s_u[j], s_u = row c of L D. The thread's largest
// |entry| and its row come back, row `c` itself left out (the first row on a tie, a NaN before any number).
template <typename T>
__device__ __forceinline__ void bk_column(const T *A, int64_t ld, T *wc, int64_t n, int64_t j0, int64_t k, int kw, int64_t c,
                                          const double *s_u, int tid, double &best, int &bi) {
  best = -1.0;
  bi = 0x7fffffff;
  for (int64_t i = k + tid; i < n; i += PT) {
    double x = i < c ? (double)A[c + i * ld] : (double)A[i + c * ld];
    const T *row = A + i + j0 * ld;
    for (int j = 0; j < kw; ++j) x = fma(-(double)row[(int64_t)j * ld], s_u[j], x);
    const T xt = (T)x;
    wc[i] = xt;
    const double a = fabs((double)xt);
    if (i != c && !(a <= best) && best == best) { best = a; bi = (int)i; }   // a NaN is taken and then kept
  }
}

__device__ __forceinline__ bool usable(double x) { return x != 0.0 && fabs(x) < __builtin_inf(); }

// perm = ipiv = 0 .. n - 1, e = 0, starts = 0, n, n, ...
__global__ void __launch_bounds__(kBlock) sytrf_init_kernel(int *__restrict__ perm, double *__restrict__ e, int64_t n, int64_t nb) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) { perm[i] = perm[n + i] = (int)i; e[i] = 0.0; }
  if (i <= nb) perm[2 * n + i] = i == 0 ? 0 : (int)n;
}

template <typename T>
__global__ void __launch_bounds__(PT) sytrf_panel_kernel(T *A, int64_t ld, int64_t n, T *Wk, int *starts, int round, int *perm,
                                                         double *d, double *e, int *info) {
  __shared__ double s_val[PT / 64], s_u[SNB];
  __shared__ int s_idx[PT / 64];
  if (*info != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int *ipiv = perm + n;
  const int64_t j0 = starts[round];
  if (j0 < 0 || j0 >= n) return;                         // the rounds before took every column: starts[round + 1] is n already
  int64_t k = j0;
  for (int step = 0; step < NB && k - j0 < NB && k < n; ++step) {
    const int kw = (int)(k - j0);
    T *w0 = Wk + (int64_t)kw * n, *w1 = w0 + n;
    if (tid < kw) s_u[tid] = (double)Wk[k + (int64_t)tid * n];
    __syncthreads();
    double cm;
    int im;
    bk_column<T>(A, ld, w0, n, j0, k, kw, k, s_u, tid, cm, im);
    panel_argmax(cm, im, s_val, s_idx, lane, wave);
    const bool below = im > k && im < n;                 // false for column n - 1 only; an index taken from data is a row
    const int64_t imax = below ? im : k;
    const double colmax = below ? cm : 0.0, absakk = fabs((double)w0[k]);
    if (!(absakk < __builtin_inf()) || !(colmax < __builtin_inf()) || (absakk == 0.0 && colmax == 0.0)) {
      if (tid == 0) *info = (int)(k + 1);
      return;
    }
    int kstep = 1;
    int64_t kp = k;
    if (!(absakk >= BK_ALPHA * colmax)) {                // only with colmax > 0, so imax is a row below k
      if (tid < kw) s_u[tid] = (double)Wk[imax + (int64_t)tid * n];
      __syncthreads();
      double rm;
      int jm;
      bk_column<T>(A, ld, w1, n, j0, k, kw, imax, s_u, tid, rm, jm);
      panel_argmax(rm, jm, s_val, s_idx, lane, wave);
      const double rowmax = (jm >= k && jm < n) ? rm : 0.0;
      if (absakk >= BK_ALPHA * colmax * (colmax / rowmax)) {
        kp = k;
      } else if (fabs((double)w1[imax]) >= BK_ALPHA * rowmax) {
        kp = imax;                                       // the diagonal entry of column imax is the 1 x 1 pivot
        for (int64_t i = k + tid; i < n; i += PT) w0[i] = w1[i];
        __syncthreads();
      } else {
        kp = imax;
        kstep = 2;
      }
    }
    const int64_t kk = k + kstep - 1;
    if (kp != kk) {                                      // kk < kp < n. Column kk of A, as the round found it, moves to place kp ...
      if (tid == 0) A[kp + kp * ld] = A[kk + kk * ld];
      for (int64_t i = kk + 1 + tid; i < kp; i += PT) A[kp + i * ld] = A[i + kk * ld];
      for (int64_t i = kp + 1 + tid; i < n; i += PT) A[i + kp * ld] = A[i + kk * ld];
      if (tid < kw) {                                    // ... rows kk and kp change places in the panel's finished columns ...
        T *c = A + (j0 + tid) * ld;
        const T x = c[kk];
        c[kk] = c[kp];
        c[kp] = x;
      }
      const int cw = tid - 2 * NB;                       // ... and in the columns 0 .. kk - j0 of L D
      if (cw >= 0 && cw <= (int)(kk - j0)) {
        T *c = Wk + (int64_t)cw * n;
        const T x = c[kk];
        c[kk] = c[kp];
        c[kp] = x;
      }
      if (tid == PT - 1) {
        const int t = perm[kk];
        perm[kk] = perm[kp];
        perm[kp] = t;
      }
    }
    if (tid == 0) {
      ipiv[k] = (int)k;
      ipiv[kk] = (int)kp;
    }
    __syncthreads();
    if (kstep == 1) {
      const T dt = w0[k];
      const double dk = (double)dt;
      if (!usable(dk)) {
        if (tid == 0) *info = (int)(k + 1);
        return;
      }
      for (int64_t i = k + 1 + tid; i < n; i += PT) A[i + k * ld] = (T)((double)w0[i] / dk);
      if (tid == 0) { A[k + k * ld] = dt; d[k] = dk; e[k] = 0.0; }
    } else {                                             // the 2 x 2 block [d0 e0; e0 d1]; L = (L D) inv(block) as in LAPACK
      const T t0 = w0[k], t1 = w1[k + 1], te = w0[k + 1];
      const double e0 = (double)te, d11 = (double)t1 / e0, d22 = (double)t0 / e0, t = d11 * d22 - 1.0;
      if (!usable(e0) || !usable(t)) {
        if (tid == 0) *info = (int)(k + 1);
        return;
      }
      const double s = (1.0 / t) / e0;
      for (int64_t i = k + 2 + tid; i < n; i += PT) {
        const double a = (double)w0[i], b = (double)w1[i];
        A[i + k * ld] = (T)(s * (d11 * a - b));
        A[i + (k + 1) * ld] = (T)(s * (d22 * b - a));
      }
      if (tid == 0) {
        A[k + k * ld] = t0;
        A[(k + 1) + k * ld] = T(0);                      // L is unit lower: the block's off-diagonal entry lives in e
        A[(k + 1) + (k + 1) * ld] = t1;
        d[k] = (double)t0; d[k + 1] = (double)t1; e[k] = e0; e[k + 1] = 0.0;
      }
    }
    __syncthreads();
    k += kstep;
  }
  if (tid == 0) starts[round + 1] = (int)k;
}

// the columns [s, j1) of round `round`, or false when there is nothing to do; both words are checked before they index anything
__device__ __forceinline__ bool panel_range(const int *starts, int round, int64_t n, int64_t &s, int64_t &j1) {
  s = starts[round];
  j1 = starts[round + 1];
  return s >= 0 && j1 > s && j1 <= n && j1 - s <= SNB;
}

// phase (b): the panel's interchanges, in order, on every column left of it; one thread a column
template <typename T>
__global__ void __launch_bounds__(kBlock) sytrf_swap_kernel(T *A, int64_t ld, int64_t n, const int *starts, int round, const int *perm,
                                                            const int *info) {
  __shared__ int sp[SNB];
  if (*info != 0) return;
  int64_t s, j1;
  if (!panel_range(starts, round, n, s, j1)) return;
  const int jb = (int)(j1 - s);
  if ((int)threadIdx.x < jb) sp[threadIdx.x] = perm[n + s + threadIdx.x];
  __syncthreads();
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= s) return;
  T *col = A + idx * ld;
  for (int p = 0; p < jb; ++p) {
    const int64_t r = sp[p];
    if (r > s + p && r < n) {
      const T x = col[s + p];
      col[s + p] = col[r];
      col[r] = x;
    }
  }
}

// phase (c): C -= P Q' on the lower triangle of the trailing matrix, P the panel of L (in A) and Q the panel of L D (in Wk):
// potrf_syrk_kernel with two operands, its sizes read from the device
template <typename T>
__global__ void __launch_bounds__(kBlock) sytrf_update_kernel(T *A, int64_t ld, int64_t n, const T *Wk, const int *starts, int round,
                                                              const int *info) {
  if (blockIdx.y > blockIdx.x) return;
  if (*info != 0) return;
  int64_t s, j1;
  if (!panel_range(starts, round, n, s, j1)) return;
  const int K = (int)(j1 - s), M = (int)(n - j1);
  const int bm = blockIdx.x * NB, bn = blockIdx.y * NB;
  if (bm >= M) return;
  T *C = A + j1 + j1 * ld;
  const T *P = A + j1 + s * ld, *Q = Wk + j1;
  __shared__ T sA[SK][SLD], sB[SK][SLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  using Acc = typename Mfma<T>::Acc;
  Acc acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[a][b][r] = 0;
  for (int k0 = 0; k0 < K; k0 += SK) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int el = tid + t * kBlock, i = el & 63, k = el >> 6, gk = k0 + k;
      sA[k][i] = (bm + i < M && gk < K) ? P[(bm + i) + (int64_t)gk * ld] : T(0);
      sB[k][i] = (bn + i < M && gk < K) ? Q[(bn + i) + (int64_t)gk * n] : T(0);
    }
    __syncthreads();
#pragma unroll
    for (int kq = 0; kq < SK; kq += 4) {
      const int kr = kq + (lane >> 4);
      const T a0 = sA[kr][wm + (lane & 15)], a1 = sA[kr][wm + 16 + (lane & 15)];
      const T b0 = sB[kr][wn + (lane & 15)], b1 = sB[kr][wn + 16 + (lane & 15)];
      acc[0][0] = Mfma<T>::run(a0, b0, acc[0][0]);
      acc[0][1] = Mfma<T>::run(a0, b1, acc[0][1]);
      acc[1][0] = Mfma<T>::run(a1, b0, acc[1][0]);
      acc[1][1] = Mfma<T>::run(a1, b1, acc[1][1]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = bm + wm + a * 16 + Mfma<T>::row(lane, r), gj = bn + wn + b * 16 + (lane & 15);
        if (gi < M && gj <= gi) {
          T *p = C + gi + (int64_t)gj * ld;
          *p = *p - acc[a][b][r];
        }
      }
}

// the inverses of all unit lower diagonal blocks of L, one workgroup each (the lower half of getrf_inv_kernel)
template <typename T>
__global__ void __launch_bounds__(kBlock) sytrf_inv_kernel(const T *__restrict__ A, int64_t ld, int64_t n, double *__restrict__ dinv,
                                                           const int *info) {
  __shared__ double sL[NB2], sX[NB2];
  if (*info != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int64_t j0 = (int64_t)blockIdx.x * NB;
  const int jb = (int)(n - j0 < NB ? n - j0 : NB);
  for (int c = q; c < NB; c += 4) {
    double x = lane == c ? 1.0 : 0.0;
    if (lane < jb && lane > c) x = (double)A[(j0 + lane) + (j0 + c) * ld];
    sL[c * NB + lane] = x;
  }
  __syncthreads();
  invert_block(sL, sX, tid, lane, q);
  double *out = dinv + (int64_t)blockIdx.x * NB2;
  for (int c = q; c < NB; c += 4) out[c * NB + lane] = sX[c * NB + lane];
}

template <typename T>
int32_t sytrf_t(mxlo_ctx *ctx, const T *M, int64_t ldm, int rowmajor, T *W, int64_t ldw, int64_t n, double *dinv, double *d, double *e,
                int *perm, T *wk, int *info_dev) {
  const int64_t nb = (n + NB - 1) / NB;
  int *starts = perm + 2 * n;
  MXLO_HIP(hipMemsetAsync(info_dev, 0, sizeof(int), ctx->stream));
  if (M) {
    hipLaunchKernelGGL((pack_upper_kernel<T>), dim3((unsigned)nb, (unsigned)nb), dim3(kBlock), 0, ctx->stream, W, ldw, M, ldm,
                       rowmajor, n);
    MXLO_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(sytrf_init_kernel, dim3((unsigned)((n + kBlock) / kBlock)), dim3(kBlock), 0, ctx->stream, perm, e, n, nb);
  MXLO_LAUNCH_CHECK();
  for (int64_t k = 0; k < nb; ++k) {
    hipLaunchKernelGGL((sytrf_panel_kernel<T>), dim3(1), dim3(PT), 0, ctx->stream, W, ldw, n, wk, starts, (int)k, perm, d, e, info_dev);
    MXLO_LAUNCH_CHECK();
    const int64_t left = k * SNB < n ? k * SNB : n;       // round k starts at column 65 k at the latest ...
    if (left > 0) {
      hipLaunchKernelGGL((sytrf_swap_kernel<T>), dim3((unsigned)((left + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, W, ldw, n,
                         (const int *)starts, (int)k, (const int *)perm, (const int *)info_dev);
      MXLO_LAUNCH_CHECK();
    }
    const int64_t m = n - (k + 1) * NB;                   // ... and ends at column 64 (k + 1) at the earliest, or at n
    if (m > 0) {
      const unsigned tiles = (unsigned)((m + NB - 1) / NB);
      hipLaunchKernelGGL((sytrf_update_kernel<T>), dim3(tiles, tiles), dim3(kBlock), 0, ctx->stream, W, ldw, n, (const T *)wk,
                         (const int *)starts, (int)k, (const int *)info_dev);
      MXLO_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL((sytrf_inv_kernel<T>), dim3((unsigned)nb), dim3(kBlock), 0, ctx->stream, (const T *)W, ldw, n, dinv,
                     (const int *)info_dev);
  MXLO_LAUNCH_CHECK();
  return MXLO_OK;
}

// z <- inv(D) z on the kb columns of z (column stride n), one launch between the two sweeps. The thread of the FIRST index of a
// pivot block handles all of it, so no thread reads an entry that another one writes; a 2 x 2 block is solved with the
// scaled explicit inverse of LAPACK's sytrs. Per entry the operations do not depend on kb.
__global__ void __launch_bounds__(kBlock) ldlp_dsolve_kernel(double *__restrict__ z, int64_t n, const double *__restrict__ d,
                                                             const double *__restrict__ e, int kb) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  if (i > 0 && e[i - 1] != 0.0) return;                  // the second index of a 2 x 2 block
  const double ei = i + 1 < n ? e[i] : 0.0;
  if (ei == 0.0) {
    const double di = d[i];
    for (int j = 0; j < kb; ++j) z[i + (int64_t)j * n] /= di;
    return;
  }
  const double akm1 = d[i] / ei, ak = d[i + 1] / ei, denom = akm1 * ak - 1.0;
  for (int j = 0; j < kb; ++j) {
    double *zj = z + i + (int64_t)j * n;
    const double bkm1 = zj[0] / ei, bk = zj[1] / ei;
    zj[0] = (ak * bkm1 - bk) / denom;
    zj[1] = (akm1 * bk - bkm1) / denom;
  }
}

// x = P L^{-T} inv(D) L^{-1} P' v: v gathered by perm, the unit lower sweep up, inv(D), the transposed sweep down with the
// epilogue scattered by perm. ceil(n / 64) + 1 + ceil(n / 64) launches.
template <typename T>
int32_t ldlp_mul_t(const Apply<T> &ap, const T *L, int64_t ld, int64_t n, const double *dinv, const double *d, const double *e,
                   const int *perm, const T *v) {
  const Tri<T> t{.Tm = L, .ld = ld, .n = n, .unit_lower = true, .dinv = dinv};
  MXLO_TRY(sweep(ap, t, {.v = v, .gather = perm}));
  hipLaunchKernelGGL(ldlp_dsolve_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, ap.ctx->stream, ap.z, n, d, e,
                     ap.grp.kb > 0 ? ap.grp.kb : 1);
  MXLO_LAUNCH_CHECK();
  return sweep(ap, t, {.trans = true, .epi = true, .scatter = perm});
}

inline int64_t sytrf_perm_bytes(int64_t n) { return (2 * n + (n + NB - 1) / NB + 1) * 4; }

int32_t ldlp_mul(mxlo_ctx *ctx, int32_t dtype, const Operands &o, const void *L, int64_t ld, int64_t n, const double *dinv, const double *d,
                 const double *e, const int32_t *perm, double *work, double alpha, double beta, const char *what) {
  bool go;
  MXLO_TRY(check_apply(ctx, dtype, o, L, ld, n, dinv, work, what, go,
                       {{d, n * 8, "the diagonal of D"}, {e, n * 8, "the sub-diagonal of D"}, {perm, n * 4, "the permutation"}}));
  if (!go) return MXLO_OK;
  MXLO_DEVICE_GUARD(ctx);
  return for_real_groups(dtype, o, [&]<typename T>(T *r, const T *v, Group grp) {
    return ldlp_mul_t<T>({ctx, r, alpha, beta, work, grp}, (const T *)L, ld, n, dinv, d, e, perm, v);
  });
}
}  // namespace

MXLO_API int32_t mxlo_sytrf(mxlo_ctx *ctx, int32_t dtype, const void *M, int64_t ldm, int32_t m_rowmajor, void *W, int64_t ldw, int64_t n,
                            double *dinv, double *d, double *e, int32_t *perm, void *panel, int32_t *info_dev, int32_t *info) {
  const char *what = "mxlo_sytrf";
  MXLO_TRY(check_common(ctx, dtype, W, ldw, n, what));
  MXLO_REQUIRE(info, MXLO_EINVAL, "%s: null info", what);
  *info = 0;
  if (n == 0) return MXLO_OK;
  MXLO_REQUIRE(dinv && d && e && perm && panel && info_dev, MXLO_EINVAL,
               "%s: null storage for the block inverses / D / the permutation / the panel workspace / the info word", what);
  MXLO_REQUIRE(n < (1LL << 31) - NB, MXLO_ESHAPE, "%s: n = %lld is too large", what, (long long)n);
  if (M) MXLO_REQUIRE(ldm >= (n > 1 ? n : 1), MXLO_ESHAPE, "%s: ldm = %lld < n", what, (long long)ldm);
  const int64_t es = esize(dtype);
  const Buf m{M, M ? mat_bytes(n, n, ldm, es) : 0, "M"};
  MXLO_TRY(disjoint({m, {W, mat_bytes(n, n, ldw, es), "the factor"}, {dinv, blocks_bytes(n), "the block inverses"},
                     {d, n * 8, "the diagonal of D"}, {e, n * 8, "the sub-diagonal of D"}, {perm, sytrf_perm_bytes(n), "the permutation"},
                     {panel, n * SNB * es, "the panel workspace"}}, what));
  MXLO_TRY(disjoint({m, {info_dev, 4, "the info word"}}, what));
  MXLO_TRY(refuse_capture(ctx, what));
  MXLO_DEVICE_GUARD(ctx);
  MXLO_TRY(with_real(dtype, [&]<typename T>() {
    return sytrf_t<T>(ctx, (const T *)M, ldm, m_rowmajor ? 1 : 0, (T *)W, ldw, n, dinv, d, e, perm, (T *)panel, info_dev);
  }));
  return read_back(ctx, info_dev, info, 1);
}

MXLO_API int32_t mxlo_ldlp_mul(mxlo_ctx *ctx, int32_t dtype, void *res, const void *L, int64_t ld, int64_t n, const double *dinv,
                               const double *d, const double *e, const int32_t *perm, double *work, const void *v, double alpha,
                               double beta) {
  return ldlp_mul(ctx, dtype, vectors(res, v, n, n), L, ld, n, dinv, d, e, perm, work, alpha, beta, "mxlo_ldlp_mul");
}

MXLO_API int32_t mxlo_ldlp_mul_block(mxlo_ctx *ctx, int32_t dtype, void *res, int64_t ldr, const void *L, int64_t ld, int64_t n,
                                     const double *dinv, const double *d, const double *e, const int32_t *perm, double *work,
                                     const void *V, int64_t ldv, int64_t k, double alpha, double beta) {
  return ldlp_mul(ctx, dtype, columns(res, ldr, V, ldv, k, n, n), L, ld, n, dinv, d, e, perm, work, alpha, beta, "mxlo_ldlp_mul_block");
}
