// Stand-alone check of the host lookahead (minesweeper-ppo_amd/csrc/mslookahead_host.h): random
// mid-game states of the two benchmark shapes (16x16x40, 30x16x99) and of two thin boards, each in
// exactly-sized heap buffers, so that a sanitizer sees any access past a board or past the K
// entries of a slot. A state is made by placing mines, opening a cell with a mine-free 3x3 around
// it, playing every provably safe cell and surviving up to three guesses, until a guess board is
// left; it is scored with random K and margin and both countings. Checked per board: candidate 0 is the
// greedy pick, the candidates are in (prob, index) order within pmin + margin, the padding is -1 /
// NaN, the choice is a candidate, a scored score lies in [0, 1 - p_c], K = 1 chooses greedily,
// and the enumerating and the grouped counting agree bit for bit. Plain C++, so it runs under
// sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iminesweeper-ppo_amd/csrc tools/mslookahead_hostcheck.cpp -o tools/bin/mslookahead_hostcheck
//   tools/bin/mslookahead_hostcheck
#include <stdio.h>
#include <string.h>

#include <memory>
#include <random>
#include <vector>

#include "mslookahead_host.h"

namespace {

struct State {
  int H, W;
  std::vector<uint8_t> mine, cnt;
  std::unique_ptr<uint8_t[]> rev, num;  // exactly H*W bytes each

  template <typename F>
  void each_nb(int i, F f) const {
    for (int dr = -1; dr <= 1; ++dr)
      for (int dc = -1; dc <= 1; ++dc) {
        const int r = i / W + dr, c = i % W + dc;
        if ((dr || dc) && r >= 0 && r < H && c >= 0 && c < W) f(r * W + c);
      }
  }
  void click(int i) {  // a safe cell: reveal it, flood fill on zeros
    std::vector<int> stack{i};
    while (!stack.empty()) {
      const int j = stack.back();
      stack.pop_back();
      if (rev[(size_t)j]) continue;
      rev[(size_t)j] = 1;
      num[(size_t)j] = cnt[(size_t)j];
      if (cnt[(size_t)j] == 0) each_nb(j, [&](int k) { if (!rev[(size_t)k]) stack.push_back(k); });
    }
  }
};

// Mines anywhere but in the 3x3 around a random opening cell, which is clicked.
State deal(int H, int W, int M, std::mt19937& rng) {
  const int A = H * W;
  State s;
  s.H = H;
  s.W = W;
  s.mine.assign((size_t)A, 0);
  s.cnt.assign((size_t)A, 0);
  const int open = (int)(rng() % (unsigned)A), orow = open / W, ocol = open % W;
  for (int placed = 0; placed < M;) {
    const int i = (int)(rng() % (unsigned)A);
    if (s.mine[(size_t)i] || (abs(i / W - orow) <= 1 && abs(i % W - ocol) <= 1)) continue;
    s.mine[(size_t)i] = 1;
    placed += 1;
  }
  for (int i = 0; i < A; ++i) s.each_nb(i, [&](int j) { s.cnt[(size_t)i] += s.mine[(size_t)j]; });
  s.rev.reset(new uint8_t[(size_t)A]());
  s.num.reset(new uint8_t[(size_t)A]);
  for (int i = 0; i < A; ++i) s.num[(size_t)i] = (uint8_t)(200 + i % 50);  // never read at hidden cells
  s.click(open);
  return s;
}

// Plays every provably safe cell until none is left; `lucky` times it then survives a guess (a
// random cell without a mine) and goes on. Returns false if a search ran out of budget or the
// game ended; otherwise the state is a guess board with posterior `prob`, `R`.
bool to_guess_board(State& s, int M, int64_t budget, int lucky, std::mt19937& rng, double* prob,
                    msposterior::Result* R, double* pmin) {
  const int A = s.H * s.W;
  for (;;) {
    *R = msposterior::analyze_grouped(s.rev.get(), s.num.get(), s.H, s.W, M, budget, prob);
    if (R->status != msposterior::kDecided) return false;
    bool any = false;
    for (int i = 0; i < A; ++i)
      if (!s.rev[(size_t)i] && prob[i] == 0.0) {
        s.click(i);
        any = true;
      }
    if (any) continue;
    if (!mslookahead::guess_board((uint8_t)R->status, prob, s.rev.get(), A, pmin)) return false;
    if (lucky-- <= 0) return true;
    std::vector<int> safe;
    for (int i = 0; i < A; ++i)
      if (!s.rev[(size_t)i] && !s.mine[(size_t)i]) safe.push_back(i);
    if (safe.empty()) return false;
    s.click(safe[rng() % safe.size()]);
  }
}

}  // namespace

int main() {
  const int shapes[][3] = {{16, 16, 40}, {16, 30, 99}, {1, 9, 2}, {7, 1, 2}};
  const int want[] = {60, 24, 12, 12};
  const int64_t budget = 1 << 12;
  std::mt19937 rng(7);
  long boards = 0, changed_boards = 0, unscored = 0, cands = 0;
  for (int si = 0; si < 4; ++si) {
    const int H = shapes[si][0], W = shapes[si][1], M = shapes[si][2], A = H * W;
    int got = 0;
    for (int tries = 0; got < want[si] && tries < 4000; ++tries) {
      State s = deal(H, W, M, rng);
      std::unique_ptr<double[]> prob(new double[(size_t)A]);
      const int Mb = M;
      msposterior::Result R;
      double pmin;
      if (!to_guess_board(s, M, budget, (int)(rng() % 4u), rng, prob.get(), &R, &pmin)) continue;
      got += 1;
      const int K = 1 + (int)(rng() % 16u);
      const double margins[] = {0.0, 0.1, 0.25, 1.0};
      const double margin = margins[rng() % 4u];
      mslookahead::Scratch scratch;
      std::unique_ptr<int32_t[]> cand(new int32_t[(size_t)K]), cand2(new int32_t[(size_t)K]);
      std::unique_ptr<double[]> score(new double[(size_t)K]), score2(new double[(size_t)K]);
      int64_t action = -7, action2 = -7;
      int32_t ns = -7, ns2 = -7;
      uint8_t ch = 7, ch2 = 7;
      mslookahead::board(prob.get(), R.configs, s.rev.get(), s.num.get(), H, W, Mb, pmin, K, margin, budget, true,
                         scratch, cand.get(), score.get(), &action, &ns, &ch);
      mslookahead::board(prob.get(), R.configs, s.rev.get(), s.num.get(), H, W, Mb, pmin, K, margin, budget, false,
                         scratch, cand2.get(), score2.get(), &action2, &ns2, &ch2);
      int greedy = -1;
      for (int c = 0; c < A && greedy < 0; ++c)
        if (!s.rev[(size_t)c] && prob[(size_t)c] == pmin) greedy = c;
      bool ok = cand[0] == greedy && ns >= 0 && ns <= K && ch <= 1;
      bool found = false;
      int counted = 0;
      for (int k = 0; k < K && ok; ++k) {
        const int c = cand[(size_t)k];
        if (c < 0) {
          ok = score[(size_t)k] != score[(size_t)k];
          for (int j = k; j < K; ++j) ok = ok && cand[(size_t)j] == -1;
          continue;
        }
        cands += 1;
        ok = c < A && !s.rev[(size_t)c] && prob[(size_t)c] <= pmin + margin;
        if (k > 0 && ok) {
          const int b = cand[(size_t)k - 1];
          ok = b >= 0 && (prob[(size_t)b] < prob[(size_t)c] || (prob[(size_t)b] == prob[(size_t)c] && b < c));
        }
        const double v = score[(size_t)k];
        if (v == v) {
          counted += 1;
          ok = ok && v >= 0.0 && v <= (1.0 - prob[(size_t)c]) * (1.0 + 1e-9);
        } else {
          unscored += 1;
        }
        found = found || c == action;
      }
      ok = ok && found && counted == ns && (ch == 1) == (action != greedy) && (K > 1 || action == greedy);
      // both countings decide these boards: the same integers, combined in the same order
      if (ns == ns2 && ok)
        ok = action == action2 && ch == ch2 && memcmp(cand.get(), cand2.get(), sizeof(int32_t) * (size_t)K) == 0 &&
             memcmp(score.get(), score2.get(), sizeof(double) * (size_t)K) == 0;
      if (!ok) {
        printf("WRONG BOARD: %dx%dx%d K %d margin %g action %lld greedy %d n_scored %d changed %d\n", H, W, Mb, K,
               margin, (long long)action, greedy, ns, (int)ch);
        return 1;
      }
      boards += 1;
      changed_boards += ch;
    }
    if (got < want[si]) {
      printf("TOO FEW GUESS BOARDS: %dx%dx%d gave %d of %d\n", H, W, M, got, want[si]);
      return 1;
    }
  }
  printf("ok: %ld guess boards, %ld candidates (%ld unscored), %ld boards with another choice than the greedy\n",
         boards, cands, unscored, changed_boards);
  return 0;
}
