/*
 * msexpert.h — C ABI of the expert policy targets derived from an exact posterior result
 * (msposterior.h / msposterior_grouped.h): per board the set of least-dangerous hidden cells, the
 * cell the greedy posterior player clicks, whether the move is provably safe or a forced guess,
 * and the per-cell mine probabilities as f32 belief targets.
 *
 * Conventions are those of msposterior.h: plain pointers, any output may be NULL, 0 (MS_OK) or an
 * MS_E* code with ms_last_error(), arguments checked before any device work. The entry points are
 * additions to ABI version 3.
 *
 * Inputs, one row per board:
 *   status u8[n]      the `status` output of any ms_posterior* call (either counting);
 *   prob f64[n,A]     its `prob` output;
 *   hidden u8[n,A]    nonzero at hidden cells (the env's action mask).
 * 1 <= A <= MS_AVOID_MAX_CELLS, 1 <= n < 2^31.
 *
 * Per board, with Hd its hidden cells:
 *   status != MS_AVOID_DECIDED, or Hd empty: the row carries no target (never a guess):
 *       kind = MS_EXPERT_NONE, best all 0, action = -1, n_best = 0, labels all 0.
 *   otherwise pmin = min over Hd of prob, and
 *     best u8[n,A]      1 exactly where the cell is hidden and prob == pmin (f64 equality);
 *     n_best i32[n]     the number of 1s in best;
 *     action i64[n]     the lowest cell index in best (the greedy pick of PosteriorModel);
 *     kind u8[n]        MS_EXPERT_SAFE if pmin == 0.0 (a provably safe move exists), else
 *                       MS_EXPERT_GUESS (every move risks a mine; best are the least dangerous);
 *     labels f32[n,A]   (float)prob at hidden cells (round to nearest, the rounding of
 *                       ms_posterior_labels' source 1), 0 elsewhere.
 *   A decided board whose hidden probabilities are all NaN (no ms_posterior* call writes one) has an
 *   empty best and is reported as MS_EXPERT_NONE with action -1; its labels keep the NaNs.
 * The computation is comparisons and one f64 -> f32 conversion: the device and the host results
 * are bitwise equal.
 */
#ifndef MSEXPERT_H
#define MSEXPERT_H

#include <stdint.h>

#include "msposterior.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MS_EXPERT_NONE 0
#define MS_EXPERT_SAFE 1
#define MS_EXPERT_GUESS 2

/* Device pointers; asynchronous on `stream`. One launch, one wavefront per board. */
int ms_expert_targets(const uint8_t* status, const double* prob, const uint8_t* hidden, int64_t n, int32_t A,
                      uint8_t* best, int64_t* action, uint8_t* kind, int32_t* n_best, float* labels,
                      void* stream);

/* The same on the host: every pointer is a HOST pointer, the call is synchronous and makes no HIP
 * call. */
int ms_expert_targets_host(const uint8_t* status, const double* prob, const uint8_t* hidden, int64_t n,
                           int32_t A, uint8_t* best, int64_t* action, uint8_t* kind, int32_t* n_best,
                           float* labels);

#ifdef __cplusplus
}
#endif

#endif /* MSEXPERT_H */
