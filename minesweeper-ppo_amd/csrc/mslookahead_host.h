// Host twin of csrc/mslookahead.hip: the two-guess lookahead of include/mslookahead.h for one
// board, in plain C++ (no HIP) on top of msposterior::analyze / analyze_grouped, so that
// tools/mslookahead_hostcheck.cpp can run it under sanitizers. It is written cell by cell with
// index lists and a sort, unlike the kernels' lane-sliced registers and wave reductions; only the
// f64 operations of the score and their order are the same, one rounding each: a product or a sum
// is a statement of its own, so that no compiler fuses two of them.
#ifndef MSLOOKAHEAD_HOST_H
#define MSLOOKAHEAD_HOST_H

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "msposterior_host.h"

namespace mslookahead {

constexpr int kMaxK = 16;       // MS_LOOKAHEAD_MAX_K
constexpr int kOutcomes = 9;    // MS_LOOKAHEAD_OUTCOMES
constexpr double kRtol = 1e-9;  // MS_LOOKAHEAD_SCORED_RTOL

// Is the board a guess board? Writes pmin when it is.
inline bool guess_board(uint8_t status, const double* prob, const uint8_t* revealed, int A, double* pmin) {
  if (status != msposterior::kDecided) return false;
  bool any = false;
  double m = INFINITY;
  for (int c = 0; c < A; ++c)
    if (!revealed[c]) {
      any = true;
      if (prob[c] < m) m = prob[c];
    }
  *pmin = m;
  return any && m > 0.0 && m < INFINITY;
}

// The candidates of a guess board into cand[K] (-1 padding); returns how many.
inline int candidates(const double* prob, const uint8_t* revealed, int A, double pmin, int K, double margin,
                      int32_t* cand) {
  const double thr = pmin + margin;
  std::vector<int> el;
  for (int c = 0; c < A; ++c)
    if (!revealed[c] && prob[c] <= thr) el.push_back(c);
  std::stable_sort(el.begin(), el.end(), [&](int a, int b) { return prob[a] < prob[b]; });
  const int nc = std::min<int>(K, (int)el.size());
  for (int k = 0; k < K; ++k) cand[k] = k < nc ? el[(size_t)k] : -1;
  return nc;
}

struct Scratch {
  std::vector<uint8_t> rev, num;
  std::vector<double> p;
};

// score(c) of one candidate of a guess board with Z layouts; returns whether c is scored.
inline bool score_candidate(const uint8_t* revealed, const uint8_t* number, int H, int W, int M, int c, double pc,
                            double Z, int64_t budget, bool grouped, Scratch& s, double* score) {
#ifdef __clang__
#pragma clang fp contract(off)  // also where this is compiled for a CPU with fused multiply-add
#endif
  const int A = H * W;
  s.rev.assign(revealed, revealed + A);
  s.num.assign(number, number + A);
  s.p.assign((size_t)A, 0.0);
  s.rev[(size_t)c] = 1;
  int hidden_nb = 0;
  const int r = c / W, col = c % W;
  for (int dr = -1; dr <= 1; ++dr)
    for (int dc = -1; dc <= 1; ++dc) {
      const int rr = r + dr, cc = col + dc;
      if ((dr || dc) && rr >= 0 && rr < H && cc >= 0 && cc < W && !revealed[rr * W + cc]) hidden_nb += 1;
    }
  double sum_z = 0.0, sum_zt = 0.0;
  for (int v = 0; v < kOutcomes && v <= hidden_nb; ++v) {
    s.num[(size_t)c] = (uint8_t)v;
    const msposterior::Result R = grouped
                                      ? msposterior::analyze_grouped(s.rev.data(), s.num.data(), H, W, M, budget, s.p.data())
                                      : msposterior::analyze(s.rev.data(), s.num.data(), H, W, M, budget, s.p.data());
    if (R.status != msposterior::kDecided) continue;  // cannot occur, or the search ran out of budget
    int hidden = 0;
    bool safe = false;
    double pm = INFINITY;
    for (int i = 0; i < A; ++i)
      if (!s.rev[(size_t)i]) {
        hidden += 1;
        if (s.p[(size_t)i] == 0.0) safe = true;
        if (s.p[(size_t)i] < pm) pm = s.p[(size_t)i];
      }
    double t = 1.0;
    if (hidden != M && !safe) t = 1.0 - pm;
    const double zt = R.configs * t;
    sum_zt = sum_zt + zt;
    sum_z = sum_z + R.configs;
  }
  const double q = 1.0 - pc;
  const double want = Z * q;
  const double diff = fabs(sum_z - want);
  const double tol = kRtol * want;
  *score = sum_zt / Z;
  return diff <= tol;
}

// The choice among nc candidates: the scored one of largest score, the earlier on ties; candidate
// 0 when none is scored. Returns the candidate's position.
inline int choose(const double* score, const uint8_t* scored, int nc) {
  int best = -1;
  for (int k = 0; k < nc; ++k)
    if (scored[k] && (best < 0 || score[k] > score[best])) best = k;
  return best < 0 ? 0 : best;
}

// One board that has a slot: cand[K], score[K] (NaN where unscored or padding) and the three
// per-board results.
inline void board(const double* prob, double Z, const uint8_t* revealed, const uint8_t* number, int H, int W, int M,
                  double pmin, int K, double margin, int64_t budget, bool grouped, Scratch& s, int32_t* cand,
                  double* score, int64_t* action, int32_t* n_scored, uint8_t* changed) {
  const int nc = candidates(prob, revealed, H * W, pmin, K, margin, cand);
  uint8_t scored[kMaxK];
  double sc[kMaxK];
  int ns = 0;
  for (int k = 0; k < K; ++k) {
    scored[k] = 0;
    sc[k] = NAN;
    if (k < nc) {
      double v;
      if (score_candidate(revealed, number, H, W, M, cand[k], prob[cand[k]], Z, budget, grouped, s, &v)) {
        scored[k] = 1;
        sc[k] = v;
        ns += 1;
      }
    }
    score[k] = sc[k];
  }
  const int pick = choose(sc, scored, nc);
  *action = cand[pick];
  *n_scored = ns;
  *changed = pick != 0 ? 1 : 0;
}

}  // namespace mslookahead

#endif  // MSLOOKAHEAD_HOST_H
