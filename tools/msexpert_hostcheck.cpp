// Stand-alone check of the host expert targets (minesweeper-ppo_amd/csrc/msexpert_host.h): random
// rows of every size 1 .. 512 in exactly-sized heap buffers, so that a sanitizer sees any access
// past a row; probabilities drawn from a small set of values (ties, exact zeros, a subnormal);
// every status; some rows with nothing hidden. Each result is checked against the definition of
// include/msexpert.h written out a second time. Plain C++, so it runs under sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iminesweeper-ppo_amd/csrc tools/msexpert_hostcheck.cpp -o tools/bin/msexpert_hostcheck
//   tools/bin/msexpert_hostcheck
#include <stdio.h>

#include <random>
#include <vector>

#include "msexpert_host.h"

int main() {
  std::mt19937 rng(1);
  const double values[] = {0.0, 4.9406564584124654e-324, 0.125, 0.25, 0.3, 0.5, 0.75, 1.0};
  long rows = 0, kinds[3] = {0, 0, 0};
  for (int A = 1; A <= 512; ++A) {
    for (int it = 0; it < 24; ++it) {
      std::vector<double> prob((size_t)A);
      std::vector<uint8_t> hidden((size_t)A), best((size_t)A, 7);
      std::vector<float> labels((size_t)A, 7.f);
      const unsigned first = rng() % 8u, span = 1u + rng() % (8u - first);
      const unsigned density = rng() % 5u;  // 0: nothing hidden
      for (int c = 0; c < A; ++c) {
        prob[(size_t)c] = values[first + rng() % span];
        hidden[(size_t)c] = density && (rng() % 4u) < density ? (uint8_t)(1u + rng() % 255u) : (uint8_t)0;
      }
      const uint8_t status = (uint8_t)(it % 6 == 5 ? rng() % 3u : 1u);
      int64_t action = 99;
      int32_t n_best = 99;
      const bool with_best = rng() % 4u != 0, with_labels = rng() % 4u != 0;
      const int kind = msexpert::board_targets(status, prob.data(), hidden.data(), A, with_best ? best.data() : nullptr,
                                               with_labels ? labels.data() : nullptr, &action, &n_best);
      // the definition, once more
      double pmin = 2.0;
      bool any = false;
      for (int c = 0; c < A; ++c)
        if (status == 1 && hidden[(size_t)c]) {
          any = true;
          if (prob[(size_t)c] < pmin) pmin = prob[(size_t)c];
        }
      int64_t want_action = -1;
      int32_t want_n = 0;
      for (int c = 0; c < A; ++c) {
        const bool b = any && hidden[(size_t)c] && prob[(size_t)c] == pmin;
        if (b && want_action < 0) want_action = c;
        want_n += b;
        const float want_label = any && hidden[(size_t)c] ? (float)prob[(size_t)c] : 0.f;
        if ((with_best && best[(size_t)c] != (b ? 1 : 0)) || (!with_best && best[(size_t)c] != 7) ||
            (with_labels && labels[(size_t)c] != want_label) || (!with_labels && labels[(size_t)c] != 7.f)) {
          printf("WRONG CELL OUTPUT: A %d row %d cell %d\n", A, it, c);
          return 1;
        }
      }
      const int want_kind = !any ? 0 : (pmin == 0.0 ? 1 : 2);
      if (kind != want_kind || action != want_action || n_best != want_n || (any && (n_best < 1 || action < 0))) {
        printf("WRONG ROW OUTPUT: A %d row %d: kind %d (want %d) action %lld (want %lld) n_best %d (want %d)\n", A, it,
               kind, want_kind, (long long)action, (long long)want_action, n_best, want_n);
        return 1;
      }
      kinds[kind] += 1;
      rows += 1;
    }
  }
  printf("ok: %ld rows of 1 .. 512 cells; kinds none / safe / guess %ld / %ld / %ld\n", rows, kinds[0], kinds[1],
         kinds[2]);
  return 0;
}
