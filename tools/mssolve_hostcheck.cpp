// Stand-alone check of the host avoidability solver (minesweeper-ppo_amd/csrc/mssolve_host.h):
// random consistent boards of the benchmark shapes and of degenerate ones (1x1, one row, one
// column, the widest board), revealed by flood fill as the game reveals them. Every cell the
// solver calls safe must be a hidden non-mine cell. Plain C++, so it runs under sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iminesweeper-ppo_amd/csrc tools/mssolve_hostcheck.cpp -o tools/bin/mssolve_hostcheck
//   tools/bin/mssolve_hostcheck
#include <stdio.h>

#include <random>
#include <vector>

#include "mssolve_host.h"

int main() {
  std::mt19937 rng(1);
  long total_safe = 0, searched = 0, max_nodes = 0;
  const int shapes[][3] = {{9, 9, 10}, {16, 16, 40}, {30, 16, 99}, {16, 30, 99},
                           {1, 1, 0},  {1, 7, 2},    {5, 1, 1},    {3, 62, 30}};
  for (const auto& s : shapes) {
    const int H = s[0], W = s[1], K = s[2], A = H * W;
    for (int it = 0; it < 150; ++it) {
      std::vector<uint8_t> mine((size_t)A, 0), rev((size_t)A, 0), safe((size_t)A);
      std::vector<int32_t> comp((size_t)A);
      for (int k = 0; k < K;) {
        const int c = (int)(rng() % (unsigned)A);
        if (!mine[(size_t)c]) {
          mine[(size_t)c] = 1;
          ++k;
        }
      }
      auto count = [&](int i) {
        int n = 0;
        for (int dr = -1; dr <= 1; ++dr)
          for (int dc = -1; dc <= 1; ++dc) {
            const int rr = i / W + dr, cc = i % W + dc;
            if ((dr || dc) && rr >= 0 && rr < H && cc >= 0 && cc < W) n += mine[(size_t)(rr * W + cc)];
          }
        return n;
      };
      const int clicks = (int)(rng() % 12u);
      for (int k = 0; k < clicks; ++k) {
        const int c = (int)(rng() % (unsigned)A);
        if (mine[(size_t)c]) continue;
        std::vector<int> stack{c};
        while (!stack.empty()) {
          const int i = stack.back();
          stack.pop_back();
          if (rev[(size_t)i]) continue;
          rev[(size_t)i] = 1;
          if (count(i)) continue;
          for (int dr = -1; dr <= 1; ++dr)
            for (int dc = -1; dc <= 1; ++dc) {
              const int rr = i / W + dr, cc = i % W + dc;
              if (rr >= 0 && rr < H && cc >= 0 && cc < W && !rev[(size_t)(rr * W + cc)]) stack.push_back(rr * W + cc);
            }
        }
      }
      const mssolve::Result R =
          mssolve::analyze(rev.data(), mine.data(), H, W, (int64_t)rng() - 1000, safe.data(), comp.data());
      int n_safe = 0;
      for (int i = 0; i < A; ++i) {
        if (safe[(size_t)i] && (mine[(size_t)i] || rev[(size_t)i])) {
          printf("UNSOUND: %dx%dx%d board %d cell %d\n", H, W, K, it, i);
          return 1;
        }
        n_safe += safe[(size_t)i];
      }
      if (n_safe != R.n_safe || (R.avoidable != 0) != (n_safe > 0)) {
        printf("INCONSISTENT: %dx%dx%d board %d\n", H, W, K, it);
        return 1;
      }
      total_safe += R.n_safe;
      searched += R.max_nodes > 0;
      if (R.max_nodes > max_nodes) max_nodes = R.max_nodes;
    }
  }
  printf("ok: %ld safe cells, %ld boards searched, largest query %ld nodes\n", total_safe, searched, max_nodes);
  return 0;
}
