// tile_div_check.cpp -- host check of tile_div (fim_kernels.h): kernel 5 turns a list
// entry's tile index into (tx, ty) with the host's multiplier and shift instead of a
// division.  For every tiles-per-row count d in 1 .. 4096 (a 65,536-cell-wide grid) and
// every tile index n below 2^25 (kTileMask + 1) it compares
//     ty = (n * mul) >> shift,   tx = n - ty * d
// with n / d and n % d; then, for larger d (every power of two up to 2^25 and its two
// neighbours), the same at the only places a monotone quotient can first go wrong: the
// last index of each row and the first of the next.  Exit status 0 = all equal.
//
//   hipcc -O2 -std=c++17 -pthread -Iinclude -Iplanning-path_planning_amd/csrc \
//         tools/tile_div_check.cpp -o tile_div_check && ./tile_div_check
// (a host program; -Xarch_host -fsanitize=address,undefined may be added.  First
// argument: the largest d of the exhaustive part, default 4096: about 1.5 minutes on
// 8 cores.)
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "fim_kernels.h"

namespace {
constexpr uint32_t kTiles = dymu::kTileMask + 1u;

bool same(uint32_t n, uint32_t d, dymu::TileDiv t) {
  const uint32_t ty = (uint32_t)(((uint64_t)n * t.mul) >> t.shift);
  const uint32_t tx = n - ty * d;
  return ty == n / d && tx == n % d;
}

// every n below 2^25
uint64_t exhaustive(uint32_t d) {
  const dymu::TileDiv t = dymu::tile_div(d);
  uint64_t bad = 0;
  for (uint32_t n = 0; n < kTiles; ++n) bad += !same(n, d, t);
  return bad;
}

// the last index of each row and the first of the next, and the range's ends
uint64_t row_ends(uint32_t d) {
  const dymu::TileDiv t = dymu::tile_div(d);
  uint64_t bad = !same(0u, d, t) + !same(kTiles - 1u, d, t);
  for (uint64_t n = d; n < kTiles; n += d) bad += !same((uint32_t)n - 1u, d, t) + !same((uint32_t)n, d, t);
  return bad;
}
}  // namespace

int main(int argc, char** argv) {
  const uint32_t dmax = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 4096u;
  unsigned nt = std::thread::hardware_concurrency();
  if (nt == 0) nt = 1;
  if (nt > 16) nt = 16;
  std::atomic<uint32_t> next{1};
  std::atomic<uint64_t> bad{0};
  std::vector<std::thread> pool;
  for (unsigned k = 0; k < nt; ++k)
    pool.emplace_back([&] {
      for (uint32_t d; (d = next.fetch_add(1)) <= dmax;) {
        const uint64_t b = exhaustive(d);
        if (b) std::fprintf(stderr, "d = %u: %llu tile indices differ\n", d, (unsigned long long)b);
        bad += b;
      }
    });
  for (auto& th : pool) th.join();
  uint64_t checked = 0;
  for (uint32_t p = 0; p <= 25; ++p)
    for (int o = -1; o <= 1; ++o) {
      const int64_t d = ((int64_t)1 << p) + o;
      if (d < 1 || d > (int64_t)kTiles) continue;
      const uint64_t b = row_ends((uint32_t)d);
      if (b) std::fprintf(stderr, "d = %lld: %llu row ends differ\n", (long long)d, (unsigned long long)b);
      bad += b;
      ++checked;
    }
  std::printf("tile_div: d = 1 .. %u exhaustively over %u tile indices, %llu further d at the row "
              "ends: %llu mismatches\n",
              dmax, kTiles, (unsigned long long)checked, (unsigned long long)bad.load());
  return bad.load() ? 1 : 0;
}
