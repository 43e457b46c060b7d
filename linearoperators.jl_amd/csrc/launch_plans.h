// launch_plans.h — the launch geometry of the dense and complex leaves (dense.hip, complex.hip), each rule stated once.
// Host code only: every function here reads its arguments and the ctx's tune keys, and touches neither the device nor the
// stream, so a host program can include this file and compare the rules over a grid of inputs (tools/launch_plans_check.cpp).
#pragma once
#include "common.h"

namespace mxlo {

// ---- GEMV, N mode: row bands --------------------------------------------------------------------------------------------
// The band height (rows per workgroup of gemv_n_rows_kernel / gemvb_n_rows_kernel / cgemv_rows_band_kernel) for an m x n
// operand of elements E, 0: keep the column-chunk schedule. VR = 16 / sizeof(E) elements per 16-byte load.
//   forced : a band height asked for by name (tune gemv_n_rows > 1, sweeps); heights other than 8 / 16 / 32 * VR give 0
//   on     : the rule below is on
//   wide_exceptions : give the wide matrices back to the column-chunk schedule. The block form passes false: the exceptions
//            weigh a finish launch that its column-chunk schedule pays KB-fold.
// The block form is bit-identical per column to the single apply only while both take the same band: one rule.
template <typename E>
inline int gemv_row_band(const void *M, int64_t m, int64_t n, int64_t ld, int num_cu, int forced, bool on,
                         bool wide_exceptions) {
  constexpr int VR = 16 / (int)sizeof(E);
  const bool vec = (((uintptr_t)M & 15u) == 0) && ld % VR == 0 && m % VR == 0;
  int rb = 0;
  if (forced) {
    if (forced == 8 * VR || forced == 16 * VR || forced == 32 * VR) rb = forced;
  } else if (on && n >= 1024) {
    // the tallest band that still gives every CU a workgroup: a band reads RB * sizeof(E) contiguous bytes per column
    // (128 B at 8 * VR), and the longer the pieces the better HBM streams them (tools/bench_gemv_n.py)
    if (m >= (int64_t)32 * VR * num_cu) rb = 32 * VR;
    else if (m >= (int64_t)16 * VR * num_cu) rb = 16 * VR;
    else if (m >= (int64_t)8 * VR * num_cu) rb = 8 * VR;
    // measured (profiles/r05_bench_gemv_n.txt): 512-byte pieces win everywhere (0.84 - 0.88 of peak); 256-byte pieces
    // win (0.78 - 0.84) except against the column-chunk schedule on very wide matrices, whose finish launch is amortised
    // there; 128-byte pieces top out at 0.68 - 0.73: better than the two launches up to n = 16384 columns only
    if (wide_exceptions) {
      if (rb == 16 * VR && n >= 16384) rb = 0;
      if (rb == 8 * VR && n > 16384) rb = 0;
    }
  }
  return (rb != 0 && vec && m >= rb) ? rb : 0;
}

// ---- GEMV, N mode: column chunks ----------------------------------------------------------------------------------------
// Workgroups of rows_per_block rows (blockIdx.x) times chunks of cpc columns (blockIdx.y), every chunk a partial sum per row:
// chunks of >= 64 columns, about 8 workgroups per CU, at most 65535 chunks, and at most max_chunk_rows partial rows in all
// (the caller's workspace, 0: no limit; m <= max_chunk_rows is the caller's check). m >= 1 and n >= 1.
struct ColChunks {
  int64_t row_blocks, nchunks, cpc;   // grid = (row_blocks, nchunks); chunk c owns columns [c * cpc, min(n, (c + 1) * cpc))
};
inline ColChunks gemv_col_chunks(int64_t m, int64_t n, int64_t rows_per_block, int num_cu, int64_t max_chunk_rows = 0) {
  ColChunks s;
  s.row_blocks = (m + rows_per_block - 1) / rows_per_block;
  s.nchunks = (n + 63) / 64;
  const int64_t want = (int64_t)num_cu * 8 / s.row_blocks + 1;
  if (s.nchunks > want) s.nchunks = want;
  if (max_chunk_rows > 0 && s.nchunks > max_chunk_rows / m) s.nchunks = max_chunk_rows / m;
  if (s.nchunks > 65535) s.nchunks = 65535;
  if (s.nchunks < 1) s.nchunks = 1;
  s.cpc = (n + s.nchunks - 1) / s.nchunks;
  s.nchunks = (n + s.cpc - 1) / s.cpc;
  return s;
}

// ---- opHermitian: tiles and strips --------------------------------------------------------------------------------------
// The strict lower triangle is cut into row groups of HR rows and tiles of HR x 32; a diagonal block is DT tiles wide and a
// workgroup owns a strip of C consecutive tiles of one row group (Q = DT / C strips across a block). The finish kernels
// index the partials by (ng, Q), the single-launch, two-launch and block forms are bit-identical to each other only while
// they agree on every count below: hermitian_t, hermitian_block_t (dense.hip) and chermitian (complex.hip) all read this.
struct HermGeom {
  bool too_large = false;   // the tile counts do not fit 31 bits: MXLO_ESHAPE "... n too large", nothing else is filled in
  int64_t ng = 0, ngf = 0;  // row groups, full row groups
  int C = 0, Q = 0;         // tiles per strip, strips across a diagonal block
  bool aligned = false;     // A takes 16-byte loads
  int64_t gi = 0;           // row groups [0, gi) run unmasked (full row groups of an aligned A), [gi, ng) masked
  int64_t n_int = 0;        // unmasked: strips strictly below the diagonal
  int64_t n_dsel = 0;       //           diagonal tiles (loaded whole, selected)
  int64_t n_all = 0;        // masked, mode 0: every strip below the diagonal (A not aligned)
  int64_t n_last = 0;       //         mode 1: the strips of the ragged last row group
  int64_t n_diag = 0;       //         mode 2: diagonal tiles of row groups gi .. ng - 1
  int64_t n_light = 0, n_edge = 0;   // grids of the unmasked and of the masked launch
};
// strip_tiles(pairs) gives C for `pairs` (row group, strip column block) pairs left of the diagonal: the real and the complex
// rule below differ.
template <typename StripRule>
inline HermGeom herm_geom(int64_t n, int HR, int DT, bool aligned, StripRule &&strip_tiles) {
  HermGeom g;
  g.ng = (n + HR - 1) / HR;
  g.ngf = n / HR;
  if (!(4 * g.ng * (g.ng + 1) < (1LL << 31))) {
    g.too_large = true;
    return g;
  }
  g.C = strip_tiles(g.ng * (g.ng - 1) / 2);
  g.Q = DT / g.C;
  g.aligned = aligned;
  g.gi = aligned ? g.ngf : 0;
  g.n_int = g.gi > 1 ? g.Q * g.gi * (g.gi - 1) / 2 : 0;
  g.n_dsel = (int64_t)DT * g.gi;
  g.n_all = !aligned && g.ng > 1 ? g.Q * g.ng * (g.ng - 1) / 2 : 0;
  g.n_last = aligned && g.ng > g.ngf ? g.Q * (g.ng - 1) : 0;
  g.n_diag = (int64_t)DT * (g.ng - g.gi);
  g.n_light = g.n_int + g.n_dsel;
  g.n_edge = g.n_all + g.n_last + g.n_diag;
  g.too_large = !(g.n_light < (1LL << 31) && g.n_edge < (1LL << 31));
  return g;
}

// Triangles small enough for the single-launch form of the real opHermitian
inline bool herm_small(const mxlo_ctx *ctx, size_t elt, int64_t n) {
  if (ctx->tune.herm_single_max_n > 0) return n <= ctx->tune.herm_single_max_n;
  return (int64_t)elt * n * (n / 2) <= ctx->tune.herm_single_max_bytes;
}
// Tiles per strip, real: 8-tile strips once there are two of them per CU, 2-tile strips with two per CU, else single tiles.
// Triangles small enough for the single-launch form (herm_small) take 2-tile strips from 1.25 per CU on — measured with the one
// launch (profiles/r06_herm_policy.txt): f64 n = 4096 14.8 -> 14.4 us, f32 n = 5120 14.1 -> 13.6; f64 n = 3072 (1.03 per CU)
// 10.1 -> 11.0: stays single tiles. The rule depends on (n, element, CUs) only, so the single launch and the two launches share
// their partial layout and stay bit-identical.
inline int herm_strip_tiles(const mxlo_ctx *ctx, size_t elt, int DT, int64_t n, int64_t pairs) {
  if (ctx->tune.herm_strip) return ctx->tune.herm_strip;
  if ((DT / 8) * pairs >= 2 * ctx->num_cu) return 8;
  if ((DT / 2) * pairs * 4 >= (herm_small(ctx, elt, n) ? 5 : 8) * (int64_t)ctx->num_cu) return 2;
  return 1;
}
// Tiles per strip, complex: whole diagonal-block-wide strips once there are two of them per CU, thinner strips below that
// (no single-launch form, and tune herm_strip is the real kernels' key)
inline int cherm_strip_tiles(const mxlo_ctx *ctx, int DT, int64_t pairs) {
  return pairs >= 2 * ctx->num_cu ? DT : ((DT / 2) * pairs >= 2 * ctx->num_cu ? 2 : 1);
}

// Cache policy of the strip loads (tune key herm_nt: -1 = this rule, 0 / 1 force): nontemporal, EXCEPT for triangles of about
// the size of the 256 MiB Infinity Cache — [herm_dp_min_bytes, herm_nt_min_bytes) = [96, 384) MiB — where the next apply of
// the same operator (a Krylov loop) finds part of a default-policy stream still there. Measured, old vs new library in one
// run (profiles/r06_herm_policy.txt): f64 n = 6144 29.8 -> 28.2 us, 8192 49.9 -> 47.3; 4096 / 5120 neutral; below (3072) the
// default policy is 10 % SLOWER, above (16384) 9 % slower.
inline bool herm_nt_policy(const mxlo_ctx *ctx, size_t elt, int64_t n) {
  if (ctx->tune.herm_nt >= 0) return ctx->tune.herm_nt != 0;
  const int64_t tri = (int64_t)elt * n * (n / 2);
  return !(tri >= ctx->tune.herm_dp_min_bytes && tri < ctx->tune.herm_nt_min_bytes);
}

// ---- MFMA GEMM (gemm_glds.h): tile class and tile parameters ------------------------------------------------------------
// Tile class for an M x N product (tools/tune_gemm.hip, profiles/r02_tune_gemm.txt): the largest tile that still gives every
// CU a workgroup — 128 with one per CU, 64 from 0.6 workgroups per CU on, else 32.
inline int gemm_tile_class(int64_t M, int64_t N, int num_cu) {
  auto tiles = [&](int t) { return ((M + t - 1) / t) * ((N + t - 1) / t); };
  if (tiles(128) >= num_cu) return 128;
  return tiles(64) * 5 >= (int64_t)num_cu * 3 ? 64 : 32;
}

// Template arguments of gemm_glds_kernel / kron_fused_kernel for a TM x TM tile class (WM x WN waves, BK-deep slabs, NST ring
// stages), per element size and A layout (a_kcontig: the factor is taken transposed, its K runs contiguously).
// PAIR (gemm_glds.h): tile pairs interleaved so that two fragments arrive with one 16-byte LDS read. Measured
// (profiles/r03_tune_gemm_pair.txt): 64-tiles -2.0 % (f64) / -2.7 % (f32), f64 128-tiles -0.6 %, f32 128-tiles +0.4 %.
// SWAPC (always on): the MFMA runs with its operands exchanged so that the accumulator holds the transposed tile and
// 16 lanes store 16 consecutive rows of the column-major C (whole 128-byte lines in f64): 1024^2 f64 72.6 -> 70.4 us,
// f32 43.1 -> 41.0 us, 2048^2 -1 ... -4 % (profiles/r03_tune_gemm_swapc.txt).
// UNR (on except for the M-contiguous f32 64- / 128-tiles, where it measured +1 ... 2 %): the steady state runs NST slabs per
// trip with the ring index a compile-time constant, so every LDS address is base + immediate and the vector ALU does no
// address work between the MFMAs: 1024^2 70.2 -> 68.9 us, the transpose mode (XOR-swizzled K-contiguous A) 79.0 -> 69.8 us,
// 32-tiles -6 ... -8 %, 128-tiles at 2048^2 -2.9 %.
// PFD 2 (fragments read two k-steps ahead): the 32-tile workgroup has ONE wave per SIMD, nothing else hides its LDS
// latency: -0.5 ... -3 % there, +1 % on the 64-tiles (two waves per SIMD) — profiles/r03_tune_gemm_bk.txt
struct GemmTile {
  int TM, WM, WN, BK, NST;
  bool PAIR;
  int PFD;
  bool UNR;
};
constexpr GemmTile gemm_tile_params(size_t elt, bool a_kcontig, int tile) {
  //                             TM  WM WN  BK NST  PAIR  PFD UNR (M-contiguous A)
  constexpr GemmTile f64[3] = {{128, 4, 4, 16, 3, true, 1, true},
                               {64, 4, 2, 32, 3, true, 1, true},
                               {32, 2, 2, 32, 4, false, 2, true}};
  constexpr GemmTile f32[3] = {{128, 4, 4, 32, 3, false, 1, false},
                               {64, 4, 2, 64, 3, true, 1, false},
                               {32, 2, 2, 64, 4, false, 2, true}};
  const int row = tile == 128 ? 0 : (tile == 64 ? 1 : 2);
  GemmTile t = elt == 8 ? f64[row] : f32[row];
  if (a_kcontig) t.UNR = true;
  return t;
}

}  // namespace mxlo
