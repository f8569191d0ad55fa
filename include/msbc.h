/* msbc.h — the behaviour-cloning minibatch loss against expert targets (msexpert.h) as two HIP
 * passes (C ABI), in the shape of msppo.h: one wavefront per minibatch row, every sum over rows
 * in a fixed order (per-workgroup partials, then one workgroup), so results are deterministic.
 *
 * Per row i, x_i are the policy logits with masked cells filled with mask_fill, log pi_i their
 * log-softmax (the masked log-softmax of msppo.h), best_i the expert's set of equally good
 * cells and w_i >= 0 the row weight (0 excludes the row: nothing of it but its weight is read
 * by the policy terms). The belief terms are those of msppo.h [3] and [4] in f32.
 *
 * Element types: logits / mine logits / labels / weight / counts are f32; action_mask, best and
 * valid are bytes (nonzero = set). The entry points are additions to ABI version 3.
 */
#ifndef MSBC_H
#define MSBC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Outputs of mc_bc_loss_fwd, f32 [8], with norm = world / counts[0] (0 when counts[0] is not > 0):
 *   [0] policy_ce = norm sum_i w_i (-(1 / n_best_i) sum_{c in best_i} log pi_i(c))
 *   [1] agree     = norm sum_i w_i [the lowest-index argmax of x_i is in best_i]   (no gradient)
 *   [2] entropy   = norm sum_i w_i (-sum_c pi_i(c) log pi_i(c))
 *   [3] aux_bce   = sum(BCEwithLogits(mine, labels, pos_weight) * valid) * world / max(counts[2], 1)
 *                   with pos_weight = (counts[2] - counts[1] + 1e-6) / (counts[1] + 1e-6)
 *   [4] aux_calib = sum((sigmoid(mine) - labels)^2 * valid) * world / max(counts[2], 1)
 *   [5] loss      = [0] - ent_coef [2] + aux_mine_weight [3] + aux_mine_calib_weight [4]
 *                   (a belief term enters only with mine given and its weight > 0)
 *   [6] bad_rows  = the number of rows with w_i != 0 whose best_i is empty or has a bit on a masked
 *                   cell, as a float (0 on clean input). Such a row's cross entropy is NaN, so [0]
 *                   and [5] are NaN, and the backward writes NaN to the row's dlogits at its legal
 *                   cells; other rows' gradients are what they are without it
 *   [7]             0 */
typedef struct {
  const float* logits;         /* [M][A] policy logits */
  const uint8_t* action_mask;  /* [M][A] nonzero = legal action */
  const uint8_t* best;         /* [M][A] nonzero = an expert cell (msexpert.h `best`) */
  const float* weight;         /* [M] row weights, >= 0 */
  const float* mine;           /* [M][A] belief logits, or NULL: no belief terms ([3], [4] = 0) */
  const float* labels;         /* [M][A] targets in [0, 1] (with mine) */
  const uint8_t* valid;        /* [M][A] cells the belief terms count, or NULL: every cell */
  const float* counts;         /* [3] (sum weight, sum labels * valid, sum valid) over the GLOBAL minibatch */
  float mask_fill;             /* the masked_fill value: -1e9 (f32 logits) or -1e4 (16-bit logits) */
  float ent_coef, aux_mine_weight, aux_mine_calib_weight;
  float world;                 /* data-parallel ranks (the counts are global) */
  int64_t M;                   /* rows of this rank's minibatch, >= 1 */
  int32_t A;                   /* actions per row = board cells, 1 ..= 512 */
} mc_bc_loss_args;

/* floats of workspace the two passes share (per-row softmax statistics + partial sums); -1 for M < 1 */
int64_t mc_bc_loss_workspace(int64_t M);

/* Forward: out f32 [8] as above (device memory); work keeps what the backward needs. */
int mc_bc_loss_fwd(const mc_bc_loss_args* a, float* out, float* work, int64_t work_floats, void* stream);

/* Backward of sum_k gout[k] out[k] (gout f32 [8] on the device): dlogits f32 [M][A] (exactly 0 at
 * masked cells and on rows of weight 0), dmine f32 [M][A] (with mine). */
int mc_bc_loss_bwd(const mc_bc_loss_args* a, const float* gout, const float* work, int64_t work_floats,
                   float* dlogits, float* dmine, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MSBC_H */
