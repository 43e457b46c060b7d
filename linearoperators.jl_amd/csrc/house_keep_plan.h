// house_keep_plan.h — how the kept form of the Householder dot launch (house_keep.h) splits a vector.
// Plain C++ with no device code, so a host program can include it on its own.
//
// The dot launch runs G workgroups over chunks of CHUNK vectors (VEC elements each) in grid-stride order: workgroup b
// takes chunks b, b + G, b + 2G, ... — "round" r is the G consecutive chunks [r G, (r + 1) G). With `rounds` complete
// rounds (every workgroup has a whole chunk), the last kl + kr of them form ONE contiguous range of the vector that the
// workgroups still hold on chip when the dot is known; they update it themselves, and so they do the short remainder
// behind the last complete round. What is left for the update launch is the prefix [0, prefix).
#pragma once
#include <cstdint>

namespace mxlo {

struct HouseKeepPlan {
  bool ok = false;        // false: fewer than two complete rounds — the form does not engage
  int64_t rounds = 0;     // complete rounds
  int64_t first = 0;      // first kept round: rounds [0, first) stream only
  int kl = 0, kr = 0;     // rounds [first, first + kl) are kept in LDS, [first + kl, rounds) in registers
  int64_t prefix = 0;     // elements [0, prefix) are left to the update launch (the scalar head included)
  int64_t rem_vec = 0;    // vectors [rem_vec, nvec) — at most one chunk per workgroup — and the scalar tail behind them
  int64_t nvec = 0;       // whole vectors behind the scalar head
};

// n elements, `head` scalar elements in front of the first 16-byte vector. KR / KL are the most rounds the kernel can
// hold in registers / LDS; with fewer complete rounds the LDS share shrinks first, and one round is always streamed.
inline HouseKeepPlan house_keep_plan(int64_t n, int64_t head, int vec, int64_t grid, int64_t chunk, int KR, int KL) {
  HouseKeepPlan p;
  if (n < head || vec < 1 || grid < 1 || chunk < 1 || KR < 0 || KL < 0) return p;
  p.nvec = (n - head) / vec;
  p.rounds = p.nvec / chunk / grid;
  if (p.rounds < 2) return p;
  const int64_t kept = p.rounds - 1 < (int64_t)KR + KL ? p.rounds - 1 : (int64_t)KR + KL;
  p.kr = (int)(kept < KR ? kept : KR);
  p.kl = (int)(kept - p.kr);
  p.first = p.rounds - kept;
  p.prefix = head + p.first * grid * chunk * vec;
  p.rem_vec = p.rounds * grid * chunk;
  p.ok = kept >= 1;
  return p;
}

// ---- a slice of h that stays in the Infinity Cache from one apply to the next -----------------------------------------
// h is the operator's own vector: every apply reads the same bytes twice (dot launch, update launch). Chunks of h marked
// "resident" are loaded with the default cache policy in both launches, every other access stays nontemporal, so once the
// slice is warm neither read of it goes to HBM. Chunks are the CHUNK-vector chunks both launches already count from
// `head`; chunk c is workgroup c % grid's chunk of round c / grid of the dot launch.

// Sixteenths of the chunks of h to keep resident for a target of `cache_bytes`: 0 for no target, 16 when all of h fits.
constexpr int house_resident_q(int64_t h_bytes, int64_t cache_bytes) {
  if (cache_bytes <= 0 || h_bytes < 0) return 0;
  if (h_bytes <= cache_bytes) return 16;
  return (int)(cache_bytes / ((h_bytes + 15) / 16));   // q/16 of h is at most the target (+ rounding of h_bytes/16)
}

// Diagonal in (round, workgroup), t = (round + workgroup) mod 16, and q of the 16 values of t spread evenly (the steps of
// floor(t q / 16)): over any 16 consecutive rounds every workgroup of the statically partitioned dot launch has exactly q
// resident chunks, and any `grid` consecutive chunks — one round — hold floor or ceil(grid q / 16) of them, so hits and
// misses are in flight together in both launches.
constexpr bool house_resident_diag(int t, int q) { return (t * q) % 16 >= 16 - q; }   // t in [0, 16), q in [0, 16]
constexpr bool house_resident_chunk(int64_t c, int64_t grid, int q) {
  return house_resident_diag((int)(((c / grid) + (c % grid)) % 16), q);
}

}  // namespace mxlo
