// Host-side check that the launch geometry of csrc/launch_plans.h is the geometry dense.hip and complex.hip computed before it was
// stated once. namespace parent holds the earlier computations as plain functions — the three column-chunk schedules (gemv_n,
// gemv_block_chunk, cgemv_rows), the three row-band rules (gemv_rows_band, the inline rule of gemv_block_chunk, cgemv_rows_band),
// the three opHermitian geometries with their cache-policy rule (hermitian_t, hermitian_block_t, chermitian) and the two tile-class
// rules (gemm, kron_t) — copied statement for statement from commit 4469fa7. main() compares every output field with the new
// functions over a grid of shapes around every threshold, CU counts, element sizes, alignments and tune values, and exits 0 when
// nothing differs. Nothing here touches a device, so the program needs no GPU. Build the host code with AddressSanitizer and UBSan
// and run it (from the repository root):
//
//   hipcc -O1 -g -std=c++20 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Iinclude tools/launch_plans_check.cpp -o /tmp/launch_plans_check && /tmp/launch_plans_check
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "../linearoperators.jl_amd/csrc/launch_plans.h"

using namespace mxlo;

namespace {
struct c64 { double re, im; };   // the sizes of Complex{Float64} / Complex{Float32}
struct c32 { float re, im; };
}  // namespace

namespace parent {
template <typename R> struct Cx;
template <> struct Cx<double> { using type = c64; };
template <> struct Cx<float> { using type = c32; };
template <typename R> using C = typename Cx<R>::type;

// ---- column chunks: what each launch received (grid.x, grid.y, the kernel's cols_per_chunk, the finish kernel's nchunks)
struct Chunks { int64_t row_blocks, nchunks, cpc; };

template <typename T>
Chunks gemv_n(const mxlo_ctx *ctx, const T *M, int64_t m, int64_t n, int64_t ld) {
  const int64_t cap = (int64_t)kMaxRedCols * kMaxRedBlocks;  // doubles in ctx->partials
  const bool pair = m >= 2 && (((uintptr_t)M % (2 * sizeof(T))) == 0) && (ld % 2 == 0);
  const int64_t rows_per_block = (int64_t)kBlock * (pair ? 2 : 1);
  const int64_t row_blocks = (m + rows_per_block - 1) / rows_per_block;
  int64_t nchunks = (n + 63) / 64;              // >= 64 columns per chunk
  const int64_t want = (int64_t)ctx->num_cu * 8 / (row_blocks > 0 ? row_blocks : 1) + 1;
  if (nchunks > want) nchunks = want;
  if (nchunks > cap / (m > 0 ? m : 1)) nchunks = cap / (m > 0 ? m : 1);
  if (nchunks < 1) nchunks = 1;
  if (nchunks > 65535) nchunks = 65535;
  const int64_t cpc = (n + nchunks - 1) / nchunks;
  nchunks = n > 0 ? (n + cpc - 1) / cpc : 1;
  return {row_blocks, nchunks, cpc > 0 ? cpc : 1};
}

template <typename T>
Chunks gemv_block_chunk(const mxlo_ctx *ctx, const T *M, int64_t m, int64_t n, int64_t ld) {
  const bool pair = m >= 2 && (((uintptr_t)M % (2 * sizeof(T))) == 0) && (ld % 2 == 0);
  const int64_t rows_per_block = (int64_t)kBlock * (pair ? 2 : 1);
  const int64_t row_blocks = (m + rows_per_block - 1) / rows_per_block;
  int64_t nchunks = (n + 63) / 64;
  const int64_t want = (int64_t)ctx->num_cu * 8 / (row_blocks > 0 ? row_blocks : 1) + 1;
  if (nchunks > want) nchunks = want;
  if (nchunks > 65535) nchunks = 65535;
  if (nchunks < 1) nchunks = 1;
  const int64_t cpc = (n + nchunks - 1) / nchunks;
  nchunks = (n + cpc - 1) / cpc;
  return {row_blocks, nchunks, cpc};
}

Chunks cgemv_rows(const mxlo_ctx *ctx, int64_t m, int64_t n) {
  const int64_t cap = (int64_t)kMaxRedCols * kMaxRedBlocks / 2;        // complex partials in ctx->partials
  const int64_t row_blocks = (m + kBlock - 1) / kBlock;
  int64_t nchunks = (n + 63) / 64;
  const int64_t want = (int64_t)ctx->num_cu * 8 / (row_blocks > 0 ? row_blocks : 1) + 1;
  if (nchunks > want) nchunks = want;
  if (nchunks > cap / (m > 0 ? m : 1)) nchunks = cap / (m > 0 ? m : 1);
  if (nchunks > 65535) nchunks = 65535;
  if (nchunks < 1) nchunks = 1;
  const int64_t cpc = n > 0 ? (n + nchunks - 1) / nchunks : 1;
  nchunks = n > 0 ? (n + cpc - 1) / cpc : 1;
  return {row_blocks, nchunks, cpc};
}

// ---- row bands
template <typename T>
int gemv_rows_band(const mxlo_ctx *ctx, const T *M, int64_t m, int64_t n, int64_t ld) {
  constexpr int VR = 16 / (int)sizeof(T);
  const bool vec = (((uintptr_t)M & 15u) == 0) && ld % VR == 0 && m % VR == 0;
  int rb = 0;
  const int want = ctx->tune.gemv_n_rows;
  if (want > 1) {
    if (want == 8 * VR || want == 16 * VR || want == 32 * VR) rb = want;
  } else if (want == 1 && n >= 1024) {
    if (m >= (int64_t)32 * VR * ctx->num_cu) rb = 32 * VR;
    else if (m >= (int64_t)16 * VR * ctx->num_cu) rb = 16 * VR;
    else if (m >= (int64_t)8 * VR * ctx->num_cu) rb = 8 * VR;
    if (rb == 16 * VR && n >= 16384) rb = 0;
    if (rb == 8 * VR && n > 16384) rb = 0;
  }
  return (rb != 0 && vec && m >= rb) ? rb : 0;
}

template <typename T>
int gemv_block_chunk_band(const mxlo_ctx *ctx, const T *M, int64_t m, int64_t n, int64_t ld) {
  constexpr int VR = 16 / (int)sizeof(T);
  const bool vec = (((uintptr_t)M & 15u) == 0) && ld % VR == 0 && m % VR == 0;
  int rb = 0;
  if (ctx->tune.gemvb_n_rows && vec && n >= 1024) {
    if (m >= (int64_t)32 * VR * ctx->num_cu) rb = 32 * VR;
    else if (m >= (int64_t)16 * VR * ctx->num_cu) rb = 16 * VR;
    else if (m >= (int64_t)8 * VR * ctx->num_cu) rb = 8 * VR;
  }
  return rb;
}

template <typename R>
int cgemv_rows_band(const mxlo_ctx *ctx, const C<R> *M, int64_t m, int64_t n, int64_t ld) {
  constexpr int VR = 16 / (int)sizeof(C<R>);
  const bool vec = (((uintptr_t)M & 15u) == 0) && ld % VR == 0 && m % VR == 0;
  if (ctx->tune.gemv_n_rows != 1 || !vec || n < 1024) return 0;
  int rb = 0;
  if (m >= (int64_t)32 * VR * ctx->num_cu) rb = 32 * VR;
  else if (m >= (int64_t)16 * VR * ctx->num_cu) rb = 16 * VR;
  else if (m >= (int64_t)8 * VR * ctx->num_cu) rb = 8 * VR;
  if (rb == 16 * VR && n >= 16384) rb = 0;
  if (rb == 8 * VR && n > 16384) rb = 0;
  return rb;
}

// ---- opHermitian
constexpr int HC = 32, CHC = 32;
template <typename T>
struct HermCfg {
  static constexpr int RPL = 16 / (int)sizeof(T);
  static constexpr int HR = 128 * RPL;
  static constexpr int DT = HR / HC;
};
template <typename R>
struct CHermCfg {
  static constexpr int RPL = 16 / (int)sizeof(C<R>);
  static constexpr int HR = 128 * RPL;
  static constexpr int DT = HR / CHC;
};
template <typename T>
inline int herm_nt_policy(const mxlo_ctx *ctx, int64_t n) {
  if (ctx->tune.herm_nt >= 0) return ctx->tune.herm_nt;
  const int64_t tri = (int64_t)sizeof(T) * n * (n / 2);
  return tri >= ctx->tune.herm_dp_min_bytes && tri < ctx->tune.herm_nt_min_bytes ? 0 : 1;
}
template <typename T>
inline bool herm_small(const mxlo_ctx *ctx, int64_t n) {
  if (ctx->tune.herm_single_max_n > 0) return n <= ctx->tune.herm_single_max_n;
  return (int64_t)sizeof(T) * n * (n / 2) <= ctx->tune.herm_single_max_bytes;
}
template <typename T>
inline int herm_strip_tiles(const mxlo_ctx *ctx, int64_t n, int64_t pairs) {
  constexpr int DT = HermCfg<T>::DT;
  if (ctx->tune.herm_strip) return ctx->tune.herm_strip;
  if ((DT / 8) * pairs >= 2 * ctx->num_cu) return 8;
  if ((DT / 2) * pairs * 4 >= (herm_small<T>(ctx, n) ? 5 : 8) * (int64_t)ctx->num_cu) return 2;
  return 1;
}

struct Herm {
  int refused = 0;          // 1 / 2: the first / second MXLO_ESHAPE check fired
  int64_t ng = 0, ngf = 0, gi = 0, n_int = 0, n_dsel = 0, n_all = 0, n_last = 0, n_diag = 0, n_light = 0, n_edge = 0;
  int C = 0, Q = 0;
  bool nt = false;
  bool single = false;      // hermitian_t: the alignment / shape part of the single-launch condition held
  int64_t n_int1 = 0, n_light1 = 0;
};

template <typename T>
Herm hermitian_t(const mxlo_ctx *ctx, const T *A, int64_t lda, int64_t n) {
  Herm h;
  constexpr int HR = HermCfg<T>::HR, DT = HermCfg<T>::DT, RPL = HermCfg<T>::RPL;
  const int64_t ng = (n + HR - 1) / HR, ngf = n / HR;
  if (!(4 * ng * (ng + 1) < (1LL << 31))) { h.refused = 1; return h; }
  const int64_t pairs = ng * (ng - 1) / 2;                       // (row group, strip column block) pairs left of the diagonal
  const int C = herm_strip_tiles<T>(ctx, n, pairs), Q = DT / C;
  const bool aligned = (((uintptr_t)A & 15u) == 0) && (lda % RPL == 0);
  const int nt = herm_nt_policy<T>(ctx, n);
  if (aligned && n % HR == 0 && herm_small<T>(ctx, n)) {
    const int64_t n_int1 = ngf > 1 ? Q * ngf * (ngf - 1) / 2 : 0, n_light1 = n_int1 + (int64_t)DT * ngf;
    h.single = true; h.n_int1 = n_int1; h.n_light1 = n_light1;
  }
  const int64_t gi = aligned ? ngf : 0;
  const int64_t n_int = gi > 1 ? Q * gi * (gi - 1) / 2 : 0;
  const int64_t n_dsel = (int64_t)DT * gi;
  const int64_t n_all = !aligned && ng > 1 ? Q * ng * (ng - 1) / 2 : 0;       // mode 0, masked
  const int64_t n_last = aligned && ng > ngf ? Q * (ng - 1) : 0;               // mode 1
  const int64_t n_diag = (int64_t)DT * (ng - gi);                              // mode 2, row groups gi .. ng-1
  const int64_t n_light = n_int + n_dsel, n_edge = n_all + n_last + n_diag;
  if (!(n_light < (1LL << 31) && n_edge < (1LL << 31))) h.refused = 2;
  h.ng = ng; h.ngf = ngf; h.gi = gi; h.n_int = n_int; h.n_dsel = n_dsel; h.n_all = n_all; h.n_last = n_last; h.n_diag = n_diag;
  h.n_light = n_light; h.n_edge = n_edge; h.C = C; h.Q = Q; h.nt = nt != 0;
  return h;
}

template <typename T>
Herm hermitian_block_t(const mxlo_ctx *ctx, const T *A, int64_t lda, int64_t n) {
  Herm h;
  constexpr int HR = HermCfg<T>::HR, DT = HermCfg<T>::DT, RPL = HermCfg<T>::RPL;
  const int64_t ng = (n + HR - 1) / HR, ngf = n / HR;
  if (!(4 * ng * (ng + 1) < (1LL << 31))) { h.refused = 1; return h; }
  const int64_t pairs = ng * (ng - 1) / 2;
  const int C = herm_strip_tiles<T>(ctx, n, pairs), Q = DT / C;
  const bool aligned = (((uintptr_t)A & 15u) == 0) && (lda % RPL == 0);
  const int nt = herm_nt_policy<T>(ctx, n);
  const int64_t gi = aligned ? ngf : 0;
  const int64_t n_int = gi > 1 ? Q * gi * (gi - 1) / 2 : 0;
  const int64_t n_dsel = (int64_t)DT * gi;
  const int64_t n_all = !aligned && ng > 1 ? Q * ng * (ng - 1) / 2 : 0;
  const int64_t n_last = aligned && ng > ngf ? Q * (ng - 1) : 0;
  const int64_t n_diag = (int64_t)DT * (ng - gi);
  const int64_t n_light = n_int + n_dsel, n_edge = n_all + n_last + n_diag;
  if (!(n_light < (1LL << 31) && n_edge < (1LL << 31))) h.refused = 2;
  h.ng = ng; h.ngf = ngf; h.gi = gi; h.n_int = n_int; h.n_dsel = n_dsel; h.n_all = n_all; h.n_last = n_last; h.n_diag = n_diag;
  h.n_light = n_light; h.n_edge = n_edge; h.C = C; h.Q = Q; h.nt = nt != 0;
  return h;
}

template <typename R>
Herm chermitian(const mxlo_ctx *ctx, const C<R> *A, int64_t lda, int64_t n) {
  Herm h;
  constexpr int HR = CHermCfg<R>::HR, DT = CHermCfg<R>::DT, RPL = CHermCfg<R>::RPL;
  const int64_t ng = (n + HR - 1) / HR, ngf = n / HR;
  if (!(4 * ng * (ng + 1) < (1LL << 31))) { h.refused = 1; return h; }
  const int64_t pairs = ng * (ng - 1) / 2;
  const int CT = pairs >= 2 * ctx->num_cu ? DT : ((DT / 2) * pairs >= 2 * ctx->num_cu ? 2 : 1), Q = DT / CT;
  const bool aligned = (((uintptr_t)A & 15u) == 0) && (lda % RPL == 0);
  const int64_t gi = aligned ? ngf : 0;
  const int64_t n_int = gi > 1 ? Q * gi * (gi - 1) / 2 : 0;
  const int64_t n_dsel = (int64_t)DT * gi;
  const int64_t n_all = !aligned && ng > 1 ? Q * ng * (ng - 1) / 2 : 0;       // mode 0, masked
  const int64_t n_last = aligned && ng > ngf ? Q * (ng - 1) : 0;               // mode 1
  const int64_t n_diag = (int64_t)DT * (ng - gi);                              // mode 2, row groups gi .. ng-1
  const int64_t n_light = n_int + n_dsel, n_edge = n_all + n_last + n_diag;
  if (!(n_light < (1LL << 31) && n_edge < (1LL << 31))) h.refused = 2;
  const int64_t tri = (int64_t)sizeof(C<R>) * n * (n / 2);
  const bool nt = ctx->tune.herm_nt >= 0 ? ctx->tune.herm_nt != 0
                                         : !(tri >= ctx->tune.herm_dp_min_bytes && tri < ctx->tune.herm_nt_min_bytes);
  h.ng = ng; h.ngf = ngf; h.gi = gi; h.n_int = n_int; h.n_dsel = n_dsel; h.n_all = n_all; h.n_last = n_last; h.n_diag = n_diag;
  h.n_light = n_light; h.n_edge = n_edge; h.C = CT; h.Q = Q; h.nt = nt;
  return h;
}

// ---- MFMA tile class: gemm() (tune gemm_tile = 0) and kron_t's tile_of
int gemm_tile(const mxlo_ctx *ctx, int64_t M, int64_t N) {
  auto tiles = [&](int tm, int tn) { return ((M + tm - 1) / tm) * ((N + tn - 1) / tn); };
  int tile = 0;
  if (tiles(128, 128) >= ctx->num_cu) tile = 128;
  else if (tiles(64, 64) * 5 >= (int64_t)ctx->num_cu * 3) tile = 64;   // >= 0.6 workgroups per CU
  else tile = 32;
  return tile;
}
int kron_tile_of(const mxlo_ctx *ctx, int64_t M, int64_t N) {
  auto tiles = [&](int tm, int tn) { return ((M + tm - 1) / tm) * ((N + tn - 1) / tn); };
  if (tiles(128, 128) >= ctx->num_cu) return 128;
  return tiles(64, 64) * 5 >= (int64_t)ctx->num_cu * 3 ? 64 : 32;
}
}  // namespace parent

// the tile parameters the launch macros of gemm() and kron_t spelled out: (TM, WM, WN, BK, NST, PAIR, PFD, UNR for M-contiguous A);
// a K-contiguous A always ran with UNR
constexpr bool same_tile(GemmTile t, int TM, int WM, int WN, int BK, int NST, bool PAIR, int PFD, bool UNR) {
  return t.TM == TM && t.WM == WM && t.WN == WN && t.BK == BK && t.NST == NST && t.PAIR == PAIR && t.PFD == PFD && t.UNR == UNR;
}
static_assert(same_tile(gemm_tile_params(8, false, 128), 128, 4, 4, 16, 3, true, 1, true) && same_tile(gemm_tile_params(8, true, 128), 128, 4, 4, 16, 3, true, 1, true));
static_assert(same_tile(gemm_tile_params(8, false, 64), 64, 4, 2, 32, 3, true, 1, true) && same_tile(gemm_tile_params(8, true, 64), 64, 4, 2, 32, 3, true, 1, true));
static_assert(same_tile(gemm_tile_params(8, false, 32), 32, 2, 2, 32, 4, false, 2, true) && same_tile(gemm_tile_params(8, true, 32), 32, 2, 2, 32, 4, false, 2, true));
static_assert(same_tile(gemm_tile_params(4, false, 128), 128, 4, 4, 32, 3, false, 1, false) && same_tile(gemm_tile_params(4, true, 128), 128, 4, 4, 32, 3, false, 1, true));
static_assert(same_tile(gemm_tile_params(4, false, 64), 64, 4, 2, 64, 3, true, 1, false) && same_tile(gemm_tile_params(4, true, 64), 64, 4, 2, 64, 3, true, 1, true));
static_assert(same_tile(gemm_tile_params(4, false, 32), 32, 2, 2, 64, 4, false, 2, true) && same_tile(gemm_tile_params(4, true, 32), 32, 2, 2, 64, 4, false, 2, true));

namespace {

int64_t compared = 0, differences = 0;
void differ(const char *what, const char *field, long long a, long long b, long long m, long long n, int cu, const char *extra = "") {
  if (++differences <= 40)
    fprintf(stderr, "DIFF %s.%s: parent %lld, here %lld  (m = %lld, n = %lld, CUs = %d%s)\n", what, field, a, b, m, n, cu, extra);
}
#define SAME(what, field, a, b, m, n, cu) \
  do { if ((long long)(a) != (long long)(b)) differ(what, field, (long long)(a), (long long)(b), m, n, cu); } while (0)

// 1 ... 70, then two either side of every value in `around` (and of 70000)
std::vector<int64_t> grid_values(const std::vector<int64_t> &around, int64_t hi) {
  std::set<int64_t> s;
  for (int64_t v = 1; v <= 70; ++v) s.insert(v);
  for (int64_t t : around)
    for (int64_t v = t - 2; v <= t + 2; ++v)
      if (v >= 1 && v <= hi) s.insert(v);
  return {s.begin(), s.end()};
}

void same_chunks(const char *what, const parent::Chunks &p, const ColChunks &c, int64_t m, int64_t n, int cu) {
  ++compared;
  SAME(what, "row_blocks", p.row_blocks, c.row_blocks, m, n, cu);
  SAME(what, "nchunks", p.nchunks, c.nchunks, m, n, cu);
  SAME(what, "cpc", p.cpc, c.cpc, m, n, cu);
}

void same_herm(const char *what, const parent::Herm &p, const HermGeom &g, bool nt, int64_t n, int cu) {
  ++compared;
  SAME(what, "too_large", p.refused != 0, g.too_large, 0, n, cu);
  if (p.refused == 1 || g.too_large) return;      // (after the first refusal nothing else was computed)
  SAME(what, "ng", p.ng, g.ng, 0, n, cu);
  SAME(what, "ngf", p.ngf, g.ngf, 0, n, cu);
  SAME(what, "C", p.C, g.C, 0, n, cu);
  SAME(what, "Q", p.Q, g.Q, 0, n, cu);
  SAME(what, "gi", p.gi, g.gi, 0, n, cu);
  SAME(what, "n_int", p.n_int, g.n_int, 0, n, cu);
  SAME(what, "n_dsel", p.n_dsel, g.n_dsel, 0, n, cu);
  SAME(what, "n_all", p.n_all, g.n_all, 0, n, cu);
  SAME(what, "n_last", p.n_last, g.n_last, 0, n, cu);
  SAME(what, "n_diag", p.n_diag, g.n_diag, 0, n, cu);
  SAME(what, "n_light", p.n_light, g.n_light, 0, n, cu);
  SAME(what, "n_edge", p.n_edge, g.n_edge, 0, n, cu);
  SAME(what, "nt", p.nt, nt, 0, n, cu);
  if (p.single) {                                  // the single launch now takes its counts from the same struct
    SAME(what, "n_int1", p.n_int1, g.n_int, 0, n, cu);
    SAME(what, "n_light1", p.n_light1, g.n_light, 0, n, cu);
  }
}

template <typename T>
HermGeom real_geom(const mxlo_ctx *ctx, const T *A, int64_t lda, int64_t n) {      // dense.hip: herm_geom_of
  using Cfg = parent::HermCfg<T>;
  const bool aligned = (((uintptr_t)A & 15u) == 0) && (lda % Cfg::RPL == 0);
  return herm_geom(n, Cfg::HR, Cfg::DT, aligned, [&](int64_t pairs) { return herm_strip_tiles(ctx, sizeof(T), Cfg::DT, n, pairs); });
}
template <typename R>
HermGeom complex_geom(const mxlo_ctx *ctx, const parent::C<R> *A, int64_t lda, int64_t n) {   // complex.hip: chermitian
  using Cfg = parent::CHermCfg<R>;
  const bool aligned = (((uintptr_t)A & 15u) == 0) && (lda % Cfg::RPL == 0);
  return herm_geom(n, Cfg::HR, Cfg::DT, aligned, [&](int64_t pairs) { return cherm_strip_tiles(ctx, Cfg::DT, pairs); });
}

// ---- per element type: T real, or R the component type of C<R>
template <typename T>
void check_real(mxlo_ctx &ctx, const std::vector<int64_t> &ms, const std::vector<int64_t> &ns, const std::vector<int64_t> &few) {
  constexpr int VR = 16 / (int)sizeof(T);
  const int64_t cap = (int64_t)kMaxRedCols * kMaxRedBlocks;
  alignas(64) static char buf[128];
  for (int mis : {0, (int)sizeof(T), 8}) {                        // 16-byte aligned; one element off; 8 bytes off
    const T *M = reinterpret_cast<const T *>(buf + mis);
    for (int64_t m : ms) {
      for (int64_t ld : {m, m + 1, m + VR, m + 2}) {
        for (int64_t n : ns) {
          // column chunks (gemv_n refuses m > cap before it gets there)
          const bool pair = m >= 2 && (((uintptr_t)M % (2 * sizeof(T))) == 0) && (ld % 2 == 0);
          if (m <= cap) same_chunks("gemv_n", parent::gemv_n<T>(&ctx, M, m, n, ld), gemv_col_chunks(m, n, (int64_t)kBlock * (pair ? 2 : 1), ctx.num_cu, cap), m, n, ctx.num_cu);
          same_chunks("gemv_block_chunk", parent::gemv_block_chunk<T>(&ctx, M, m, n, ld), gemv_col_chunks(m, n, (int64_t)kBlock * (pair ? 2 : 1), ctx.num_cu), m, n, ctx.num_cu);
          // row bands: rule off / on here, every forced height below on the short list
          for (int want : {0, 1}) {
            ctx.tune.gemv_n_rows = want;
            ++compared;
            SAME("gemv_rows_band", "rb", parent::gemv_rows_band<T>(&ctx, M, m, n, ld), gemv_row_band<T>(M, m, n, ld, ctx.num_cu, want > 1 ? want : 0, want == 1, true), m, n, ctx.num_cu);
            ctx.tune.gemvb_n_rows = want;
            ++compared;
            SAME("gemv_block_chunk band", "rb", parent::gemv_block_chunk_band<T>(&ctx, M, m, n, ld), gemv_row_band<T>(M, m, n, ld, ctx.num_cu, 0, ctx.tune.gemvb_n_rows != 0, false), m, n, ctx.num_cu);
          }
        }
      }
    }
    for (int want = 0; want <= 128; ++want) {                     // every accepted gemv_n_rows
      ctx.tune.gemv_n_rows = want;
      for (int64_t m : few)
        for (int64_t ld : {m, m + 1, m + VR})
          for (int64_t n : few) {
            ++compared;
            SAME("gemv_rows_band (forced)", "rb", parent::gemv_rows_band<T>(&ctx, M, m, n, ld), gemv_row_band<T>(M, m, n, ld, ctx.num_cu, want > 1 ? want : 0, want == 1, true), m, n, ctx.num_cu);
          }
    }
    ctx.tune.gemv_n_rows = 1;
    ctx.tune.gemvb_n_rows = 1;
  }
}

template <typename R>
void check_complex(mxlo_ctx &ctx, const std::vector<int64_t> &ms, const std::vector<int64_t> &ns, const std::vector<int64_t> &few) {
  using E = parent::C<R>;
  constexpr int VR = 16 / (int)sizeof(E);
  const int64_t cap = (int64_t)kMaxRedCols * kMaxRedBlocks / 2;
  alignas(64) static char buf[128];
  for (int mis : {0, 8}) {
    const E *M = reinterpret_cast<const E *>(buf + mis);
    for (int64_t m : ms)
      for (int64_t ld : {m, m + 1, m + VR})
        for (int64_t n : ns) {
          if (m <= cap && mis == 0 && ld == m) same_chunks("cgemv_rows", parent::cgemv_rows(&ctx, m, n), gemv_col_chunks(m, n, kBlock, ctx.num_cu, cap), m, n, ctx.num_cu);
          for (int want : {0, 1}) {
            ctx.tune.gemv_n_rows = want;
            ++compared;
            SAME("cgemv_rows_band", "rb", parent::cgemv_rows_band<R>(&ctx, M, m, n, ld), gemv_row_band<E>(M, m, n, ld, ctx.num_cu, 0, ctx.tune.gemv_n_rows == 1, true), m, n, ctx.num_cu);
          }
        }
    for (int want = 0; want <= 128; ++want) {
      ctx.tune.gemv_n_rows = want;
      for (int64_t m : few)
        for (int64_t n : few) {
          ++compared;
          SAME("cgemv_rows_band (forced)", "rb", parent::cgemv_rows_band<R>(&ctx, M, m, n, m), gemv_row_band<E>(M, m, n, m, ctx.num_cu, 0, ctx.tune.gemv_n_rows == 1, true), m, n, ctx.num_cu);
        }
    }
    ctx.tune.gemv_n_rows = 1;
  }
}

template <typename T, typename R>
void check_herm(mxlo_ctx &ctx, const std::vector<int64_t> &hn) {
  alignas(64) static char buf[128];
  for (int strip : {0, 1, 2, 8})
    for (int nt : {-1, 0, 1})
      for (int mis : {0, 8}) {
        ctx.tune.herm_strip = strip;
        ctx.tune.herm_nt = nt;
        const T *A = reinterpret_cast<const T *>(buf + mis);
        const parent::C<R> *Ac = reinterpret_cast<const parent::C<R> *>(buf + mis);
        for (int64_t n : hn)
          for (int64_t lda : {n, n + 1, n + 2, n + 4}) {
            const HermGeom g = real_geom<T>(&ctx, A, lda, n);
            const bool pol = herm_nt_policy(&ctx, sizeof(T), n);
            same_herm("hermitian_t", parent::hermitian_t<T>(&ctx, A, lda, n), g, pol, n, ctx.num_cu);
            same_herm("hermitian_block_t", parent::hermitian_block_t<T>(&ctx, A, lda, n), g, pol, n, ctx.num_cu);
            same_herm("chermitian", parent::chermitian<R>(&ctx, Ac, lda, n), complex_geom<R>(&ctx, Ac, lda, n),
                      herm_nt_policy(&ctx, sizeof(parent::C<R>), n), n, ctx.num_cu);
          }
      }
  ctx.tune.herm_strip = 0;
  ctx.tune.herm_nt = -1;
}

}  // namespace

int main() {
  mxlo_ctx ctx;                                   // the tune defaults of tune_keys.def; no device, no stream
  const int64_t cap = (int64_t)kMaxRedCols * kMaxRedBlocks;
  for (int cu : {1, 8, 64, 256, 304}) {
    ctx.num_cu = cu;
    std::vector<int64_t> around = {kBlock, 2 * kBlock, 1024, 16384, 65535, 70000};
    for (int vr : {1, 2, 4})
      for (int h : {8, 16, 32}) around.push_back((int64_t)h * vr * cu);
    for (int64_t rb = 1; rb <= 4; ++rb) around.push_back((int64_t)cu * 8 / rb * 64);   // where `want` chunks of 64 columns end
    const std::vector<int64_t> ns = grid_values(around, 70000);
    std::vector<int64_t> around_m = around;
    for (int64_t c = 2; c <= 8; ++c) around_m.push_back(cap / c);                      // where the workspace cap cuts nchunks
    around_m.push_back(cap / 16);
    std::vector<int64_t> ms = grid_values(around_m, 70000);
    for (int64_t v : {cap / 2 - 1, cap / 2, cap / 2 + 1, cap - 1, cap, cap + 1}) ms.push_back(v);   // the largest m the callers pass
    std::vector<int64_t> few;
    for (int64_t v : grid_values({1024, 16384, (int64_t)8 * cu, (int64_t)16 * cu, (int64_t)64 * cu, (int64_t)128 * cu}, 70000))
      if (v <= 4 || v > 70 || v % 16 == 0) few.push_back(v);
    check_real<double>(ctx, ms, ns, few);
    check_real<float>(ctx, ms, ns, few);
    check_complex<double>(ctx, ms, ns, few);
    check_complex<float>(ctx, ms, ns, few);

    // opHermitian: n around every row-group multiple that changes the strip rule, the policy windows and both refusals
    std::vector<int64_t> ha = {128, 256, 512, 1024, 2048, 3072, 4096, 5120, 6144, 8192, 16384, 32768, 65536, 70000};
    for (int64_t hr : {128, 256, 512})
      for (int64_t ng : {2, 3, 4, 5, 8, 12, 16, 17, 23, 24, 32, 33, 45, 46, 64, 90, 91, 128}) ha.push_back(hr * ng);
    std::vector<int64_t> hn = grid_values(ha, 70000);
    for (int64_t hr : {128, 256, 512})                            // 4 ng (ng + 1) reaches 2^31 at ng = 23170; 8 ng^2 at ng = 16384
      for (int64_t ng : {16383, 16384, 16385, 23169, 23170, 23171})
        for (int64_t d : {-1, 0, 1}) hn.push_back(hr * ng + d);
    for (int64_t single_n : {(int64_t)0, (int64_t)4096}) {        // herm_small by bytes (default) and by n
      ctx.tune.herm_single_max_n = single_n;
      check_herm<double, double>(ctx, hn);
      check_herm<float, float>(ctx, hn);
    }
    ctx.tune.herm_single_max_n = 0;

    // MFMA tile class
    for (int64_t M : ns)
      for (int64_t N : ns) {
        if (M > 20000 && N > 20000) continue;
        compared += 2;
        const int t = gemm_tile_class(M, N, cu);
        SAME("gemm", "tile", parent::gemm_tile(&ctx, M, N), t, M, N, cu);
        SAME("kron_t", "tile_of", parent::kron_tile_of(&ctx, M, N), t, M, N, cu);
      }
  }
  printf("inputs compared: %lld, differences: %lld\n", (long long)compared, (long long)differences);
  return differences == 0 ? 0 : 1;
}
