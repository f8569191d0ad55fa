// Stand-alone check of the grouped host posterior solver (msposterior::analyze_grouped of
// minesweeper-ppo_amd/csrc/msposterior_host.h), in the manner of tools/msposterior_hostcheck.cpp:
// random consistent boards of the benchmark shapes and of degenerate ones (1x1, one row, one
// column, the widest board), revealed by flood fill as the game reveals them. On every board the
// grouped solver decides, the probabilities lie in [0, 1], sum to the mine count within 1e-9, are
// 0 at revealed cells and positive at every true mine; wherever the enumerating solver decides
// too, prob and configs are bitwise equal. Plain C++, so it runs under sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iminesweeper-ppo_amd/csrc tools/msposterior_grouped_hostcheck.cpp -o tools/bin/msposterior_grouped_hostcheck
//   tools/bin/msposterior_grouped_hostcheck
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "msposterior_host.h"

int main() {
  std::mt19937 rng(1);
  long decided = 0, undecided = 0, skipped = 0, max_nodes = 0, both = 0, enum_only = 0, enum_undecided = 0, enum_max = 0;
  double worst_sum = 0.0;
  const int64_t budget = 1 << 16;
  const int shapes[][4] = {{9, 9, 10, 150}, {16, 16, 40, 150}, {30, 16, 99, 40}, {16, 30, 99, 40},
                           {1, 1, 0, 20},   {1, 7, 2, 150},    {5, 1, 1, 150},   {3, 62, 30, 60}};
  for (const auto& s : shapes) {
    const int H = s[0], W = s[1], K = s[2], A = H * W;
    for (int it = 0; it < s[3]; ++it) {
      std::vector<uint8_t> mine((size_t)A, 0), rev((size_t)A, 0), num((size_t)A, 0);
      std::vector<double> p((size_t)A), pe((size_t)A);
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
          num[(size_t)i] = (uint8_t)count(i);
          if (num[(size_t)i]) continue;
          for (int dr = -1; dr <= 1; ++dr)
            for (int dc = -1; dc <= 1; ++dc) {
              const int rr = i / W + dr, cc = i % W + dc;
              if (rr >= 0 && rr < H && cc >= 0 && cc < W && !rev[(size_t)(rr * W + cc)]) stack.push_back(rr * W + cc);
            }
        }
      }
      for (int i = 0; i < A; ++i)
        if (!rev[(size_t)i]) num[(size_t)i] = (uint8_t)(rng() % 9u);  // must never be read
      const msposterior::Result R = msposterior::analyze_grouped(rev.data(), num.data(), H, W, K, budget, p.data());
      const msposterior::Result E = msposterior::analyze(rev.data(), num.data(), H, W, K, budget, pe.data());
      if (R.max_nodes > max_nodes) max_nodes = R.max_nodes;
      if (E.status == msposterior::kDecided && E.max_nodes > enum_max) enum_max = E.max_nodes;
      enum_undecided += E.status == msposterior::kUndecided;
      if ((R.status == msposterior::kSkipped) != (E.status == msposterior::kSkipped)) {
        printf("SKIPPED by one method only: %dx%dx%d board %d\n", H, W, K, it);
        return 1;
      }
      if (E.status == msposterior::kDecided && R.status != msposterior::kDecided) enum_only += 1;
      if (E.status == msposterior::kDecided && R.status == msposterior::kDecided) {
        if (memcmp(&R.configs, &E.configs, sizeof(double)) != 0 ||
            memcmp(p.data(), pe.data(), sizeof(double) * (size_t)A) != 0) {
          printf("NOT BITWISE EQUAL to the enumerating solver: %dx%dx%d board %d (configs %.17g vs %.17g)\n", H, W, K, it,
                 R.configs, E.configs);
          return 1;
        }
        both += 1;
      }
      if (R.status == msposterior::kSkipped || R.status == msposterior::kUndecided) {
        bool any_rev = false;
        for (int i = 0; i < A; ++i) any_rev |= rev[(size_t)i] != 0;
        if ((R.status == msposterior::kSkipped) == any_rev) {
          printf("WRONG STATUS %d: %dx%dx%d board %d\n", R.status, H, W, K, it);
          return 1;
        }
        for (int i = 0; i < A; ++i)
          if (p[(size_t)i] != 0.0) {
            printf("NONZERO OUTPUT without a decision: %dx%dx%d board %d cell %d\n", H, W, K, it, i);
            return 1;
          }
        (R.status == msposterior::kSkipped ? skipped : undecided) += 1;
        continue;
      }
      if (R.status != msposterior::kDecided || !(R.configs >= 1.0)) {
        printf("INCONSISTENT verdict on a consistent board: %dx%dx%d board %d\n", H, W, K, it);
        return 1;
      }
      double sum = 0.0;
      for (int i = 0; i < A; ++i) {
        const double v = p[(size_t)i];
        if (!(v >= 0.0 && v <= 1.0) || (rev[(size_t)i] && v != 0.0) || (mine[(size_t)i] && !(v > 0.0))) {
          printf("BAD PROBABILITY %g: %dx%dx%d board %d cell %d (revealed %d, mine %d)\n", v, H, W, K, it, i,
                 rev[(size_t)i], mine[(size_t)i]);
          return 1;
        }
        sum += v;
      }
      if (fabs(sum - K) > 1e-9) {
        printf("SUM %0.12f != %d: %dx%dx%d board %d\n", sum, K, H, W, K, it);
        return 1;
      }
      if (fabs(sum - K) > worst_sum) worst_sum = fabs(sum - K);
      decided += 1;
    }
  }
  printf("ok: grouped %ld boards decided, %ld undecided at 2^16 nodes, %ld skipped, largest query %ld nodes, "
         "worst |sum p - M| %.3g; enumerate %ld undecided at 2^16 nodes (largest decided query %ld), %ld boards "
         "decided by both and bitwise equal, %ld by enumerate only\n",
         decided, undecided, skipped, max_nodes, worst_sum, enum_undecided, enum_max, both, enum_only);
  return 0;
}
