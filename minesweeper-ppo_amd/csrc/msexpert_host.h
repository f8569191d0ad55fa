// Host twin of k_expert (csrc/msexpert.hip): the expert targets of include/msexpert.h for one
// board, in plain C++ (no HIP), so that tools/msexpert_hostcheck.cpp can run it under sanitizers.
#ifndef MSEXPERT_HOST_H
#define MSEXPERT_HOST_H

#include <math.h>
#include <stdint.h>

namespace msexpert {

// One board: status, prob [A], hidden [A] -> best [A], labels [A] (either may be null) and the
// three per-board results. Returns the board's kind (0 none, 1 safe, 2 guess).
inline int board_targets(uint8_t status, const double* prob, const uint8_t* hidden, int A, uint8_t* best,
                         float* labels, int64_t* action, int32_t* n_best) {
  bool any = false;
  double pmin = INFINITY;
  if (status == 1)  // MS_AVOID_DECIDED
    for (int c = 0; c < A; ++c)
      if (hidden[c]) {
        any = true;
        if (prob[c] < pmin) pmin = prob[c];
      }
  int64_t act = -1;
  int32_t nb = 0;
  for (int c = 0; c < A; ++c) {
    const bool b = any && hidden[c] && prob[c] == pmin;
    if (b) {
      if (act < 0) act = c;
      ++nb;
    }
    if (best) best[c] = b ? 1 : 0;
    if (labels) labels[c] = (any && hidden[c]) ? (float)prob[c] : 0.f;
  }
  *action = act;
  *n_best = nb;
  return nb == 0 ? 0 : (pmin == 0.0 ? 1 : 2);
}

}  // namespace msexpert

#endif  // MSEXPERT_HOST_H
