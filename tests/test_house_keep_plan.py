"""The split of a vector by the kept form of the Householder dot launch (csrc/house_keep_plan.h), checked on the host:
a stand-alone C++ program includes the header, is built with the address and undefined-behaviour sanitizers and walks
every n from 1 to a few thousand chunks' worth for small synthetic grids."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "linearoperators.jl_amd", "csrc")

PROGRAM = r"""
#include "house_keep_plan.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using mxlo::HouseKeepPlan;

#define REQUIRE(c)                                                                                              \
  do {                                                                                                          \
    if (!(c)) {                                                                                                 \
      std::printf("FAIL %s: G=%lld CHUNK=%lld VEC=%d head=%lld KR=%d KL=%d n=%lld\n", #c, (long long)G,          \
                  (long long)CHUNK, VEC, (long long)head, KR, KL, (long long)n);                                \
      return 1;                                                                                                 \
    }                                                                                                           \
  } while (0)

// Workgroup b's i-th chunk in grid-stride order is b + i G. `per_wg`: also walk every workgroup's chunks.
static int check(int64_t G, int64_t CHUNK, int VEC, int64_t head, int KR, int KL, int64_t n, bool per_wg, long *engaged) {
  const HouseKeepPlan p = mxlo::house_keep_plan(n, head, VEC, G, CHUNK, KR, KL);
  const int64_t nvec = n >= head ? (n - head) / VEC : 0, rounds = nvec / CHUNK / G;
  if (rounds < 2) {
    REQUIRE(!p.ok);
    return 0;
  }
  ++*engaged;
  REQUIRE(p.ok && p.nvec == nvec && p.rounds == rounds);
  REQUIRE(p.kr >= 0 && p.kr <= KR && p.kl >= 0 && p.kl <= KL && p.kr + p.kl >= 1);
  REQUIRE(p.first >= 1 && p.first + p.kl + p.kr == rounds);                       // one streamed round at least
  REQUIRE(p.kr + p.kl == (rounds - 1 < KR + KL ? rounds - 1 : KR + KL));          // shrinks only when it must
  // prefix (update launch), kept rounds, remainder vectors and scalar tail follow each other from 0 to n without a gap
  const int64_t round_elems = G * CHUNK * VEC, kept = p.kl + p.kr;
  int64_t pos = p.prefix;
  REQUIRE(p.prefix == head + p.first * round_elems);
  for (int64_t q = 0; q < kept; ++q) {
    REQUIRE(head + (p.first + q) * round_elems == pos);
    pos += round_elems;
  }
  REQUIRE(head + p.rem_vec * VEC == pos && nvec >= p.rem_vec && nvec - p.rem_vec < G * CHUNK);
  pos += (nvec - p.rem_vec) * VEC;
  REQUIRE(pos == head + nvec * VEC && n >= pos && n - pos < VEC);
  if (!per_wg) return 0;
  const int64_t nchunks = (nvec + CHUNK - 1) / CHUNK;
  int64_t covered = 0;
  for (int64_t b = 0; b < G; ++b) {
    const int64_t mine = (nchunks - b + G - 1) / G;                               // chunks b, b + G, ... < nchunks
    REQUIRE(mine == rounds || mine == rounds + 1);
    for (int64_t q = 0; q < kept; ++q) {                                           // its last `kept` WHOLE-round chunks, in order
      const int64_t ch = (p.first + q) * G + b;
      REQUIRE(ch == b + (rounds - kept + q) * G && (ch + 1) * CHUNK <= nvec);
      covered += CHUNK;
    }
    const int64_t r0 = p.rem_vec + b * CHUNK;                                      // at most one chunk behind them
    const int64_t rn = r0 >= nvec ? 0 : (nvec - r0 < CHUNK ? nvec - r0 : CHUNK);
    REQUIRE((rn > 0) == (mine == rounds + 1));
    if (rn > 0) REQUIRE(r0 == (b + rounds * G) * CHUNK);
    covered += rn;
  }
  REQUIRE(covered == nvec - p.first * G * CHUNK);
  return 0;
}

int main() {
  long engaged = 0, total = 0;
  const int kept[4][2] = {{14, 4}, {12, 4}, {8, 0}, {2, 1}};
  for (int VEC : {2, 4})
    for (int64_t head : {0, 1})
      for (const auto &k : kept) {
        // G = 4, CHUNK = 8: every n up to 3000 chunks' worth, every workgroup walked
        for (int64_t n = 1; n <= 3000 * 8 * VEC + 7; ++n, ++total)
          if (check(4, 8, VEC, head, k[0], k[1], n, true, &engaged)) return 1;
        // G = 256, CHUNK = 1024 with the shipped constants: every n up to 3000 chunks' worth (11 rounds), the workgroups
        // walked at a sample of them
        for (int64_t n = 1; k == kept[0] && n <= 3000 * 1024 * VEC + 7; ++n, ++total) {
          const int64_t m = n % (1024 * VEC);
          if (check(256, 1024, VEC, head, k[0], k[1], n, m < 3 || m > 1024 * VEC - 3 || n % 65537 == 0, &engaged)) return 1;
        }
      }
  // ... and the shipped grid at more rounds than it keeps
  for (int VEC : {2, 4})
    for (int64_t head : {0, 1})
      for (int rounds = 14; rounds <= 26; ++rounds)
        for (int64_t extra : {(int64_t)0, (int64_t)1, (int64_t)1023 * VEC + 1, (int64_t)256 * 1024 * VEC - 1}) {
          ++total;
          if (check(256, 1024, VEC, head, 14, 4, head + (int64_t)rounds * 256 * 1024 * VEC + extra, true, &engaged)) return 1;
        }
  std::printf("OK %ld plans, %ld engaged\n", total, engaged);
  return engaged > 1000 ? 0 : 1;
}
"""


def test_plan_tiles_the_vector_exactly_once_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = tmp_path / "plan_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "plan_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", HEADER_DIR, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith("OK"), run.stdout[-2000:] + run.stderr[-4000:]
