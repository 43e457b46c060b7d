"""The rule that picks the slice of h kept in the Infinity Cache (csrc/house_keep_plan.h: house_resident_q,
house_resident_chunk), checked on the host: a stand-alone C++ program includes the header, is built with the address and
undefined-behaviour sanitizers and walks grids, q and rounds."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "linearoperators.jl_amd", "csrc")

PROGRAM = r"""
#include "house_keep_plan.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
using mxlo::house_resident_chunk;
using mxlo::house_resident_q;

#define REQUIRE(c)                                                                                          \
  do {                                                                                                      \
    if (!(c)) {                                                                                             \
      std::printf("FAIL %s: grid=%lld q=%d a=%lld b=%lld\n", #c, (long long)grid, q, (long long)a, (long long)b); \
      return 1;                                                                                             \
    }                                                                                                       \
  } while (0)

int main() {
  long checked = 0;
  const int64_t ROUNDS = 96;
  for (int64_t grid : {1, 7, 256, 304})
    for (int q = 0; q <= 16; ++q) {
      int64_t a = 0, b = 0;
      std::vector<std::vector<char>> m(ROUNDS, std::vector<char>(grid));
      for (int64_t r = 0; r < ROUNDS; ++r)
        for (int64_t w = 0; w < grid; ++w) m[r][w] = house_resident_chunk(r * grid + w, grid, q) ? 1 : 0;
      // every workgroup has the same resident count over ANY 16 consecutive rounds: q of them
      for (int64_t r0 = 0; r0 + 16 <= ROUNDS; ++r0)
        for (int64_t w = 0; w < grid; ++w) {
          int cnt = 0;
          for (int64_t r = r0; r < r0 + 16; ++r) cnt += m[r][w];
          a = r0, b = w;
          REQUIRE(cnt == q);
          ++checked;
        }
      // every round has round(grid q / 16) +- 1 resident chunks; q = 0 marks none, q = 16 marks all
      const long want = std::lround((double)grid * q / 16.0);
      for (int64_t r = 0; r < ROUNDS; ++r) {
        long cnt = 0;
        for (int64_t w = 0; w < grid; ++w) cnt += m[r][w];
        a = r, b = cnt;
        REQUIRE(cnt >= want - 1 && cnt <= want + 1);
        if (q == 0) REQUIRE(cnt == 0);
        if (q == 16) REQUIRE(cnt == grid);
        ++checked;
      }
    }
  // house_resident_q: 0 for no target, 16 when all of h fits, monotone in the target, never more than the target holds
  {
    const int64_t grid = 0;
    int q = 0;
    for (int64_t hb : {(int64_t)1, (int64_t)15, (int64_t)16, (int64_t)17, (int64_t)4096, (int64_t)800000000, (int64_t)400000000,
                       (int64_t)1 << 28, ((int64_t)1 << 40) + 8}) {
      int64_t a = hb, b = 0;
      REQUIRE(house_resident_q(hb, 0) == 0);
      REQUIRE(house_resident_q(hb, hb) == 16 && house_resident_q(hb, hb + 1) == 16);
      int prev = 0;
      for (int k = 0; k <= 4096; ++k) {                     // targets from 0 to a little over h_bytes
        b = (int64_t)((long double)hb * k / 4000);
        q = house_resident_q(hb, b);
        REQUIRE(q >= prev && q >= 0 && q <= 16);
        REQUIRE((q == 16) == (hb <= b && b > 0));
        if (q < 16) REQUIRE((long double)q * hb / 16 <= (long double)b);
        prev = q;
        ++checked;
      }
    }
    int64_t a = 0, b = 0;
    REQUIRE(house_resident_q(800000000, (int64_t)192 << 20) == 4);      // the headline: 200 MB of h
    REQUIRE(house_resident_q((int64_t)1 << 28, (int64_t)192 << 20) == 12);
  }
  std::printf("OK %ld checks\n", checked);
  return checked > 10000 ? 0 : 1;
}
"""


def test_resident_rule_is_diagonal_and_even_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = tmp_path / "resident_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "resident_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", HEADER_DIR, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith("OK"), run.stdout[-2000:] + run.stderr[-4000:]
