/*
 * msposterior_labels.h — C ABI of the exact posterior as training targets of the belief head:
 * msposterior.h's analysis of a handle's boards, written in the layout of ms_labels (msenv.h).
 * Conventions are those of msposterior.h. The entry point is an addition to ABI version 3.
 */
#ifndef MSPOSTERIOR_LABELS_H
#define MSPOSTERIOR_LABELS_H

#include <stdint.h>

#include "msposterior.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ms_posterior's analysis of the handle's boards as they stand, written as training targets of
 * the belief head in the layout of ms_labels' two outputs (one launch, one wavefront per board,
 * the search of ms_posterior with another output stage). budget: nodes per query, 1 <= budget <= 2^30; the
 * handle's ms_posterior_set_budget value is neither read nor changed. Outputs (any may be NULL):
 *   labels f32[n,H*W]  by `source`, below;
 *   valid u8[n,H*W]    what ms_labels writes: 1 at hidden cells once the first click is done,
 *                      else 0;
 *   source u8[n]       0 before the first click: labels are 0, as ms_labels writes;
 *                      1 decided: labels[i] = (float)p[i], the f64 posterior rounded to nearest
 *                        (0 at revealed cells);
 *                      2 not decided (budget, a component of more than MS_AVOID_MAX_VARS free
 *                        cells, more than MS_AVOID_MAX_CELLS cells, an inconsistent board): labels
 *                        are the 0 / 1 mine mask, bit for bit what ms_labels writes;
 *   max_nodes i32[n]   as ms_posterior's.
 * Never a zero row or a guess: the mine mask is itself one sample of the posterior, so a batch
 * of mixed sources stays an unbiased target. Reads only, as ms_posterior. */
int ms_posterior_labels(ms_handle* h, int32_t budget, float* labels, uint8_t* valid,
                        uint8_t* source, int32_t* max_nodes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MSPOSTERIOR_LABELS_H */
