/*
 * msdagger.h — C ABI of the action mix of on-policy imitation (DAgger): per board, who plays the
 * next move — the teacher (the expert action of msexpert.h), the learner (its own logits, greedy
 * or sampled) or a uniform legal click — decided by two keyed coins, in one launch.
 *
 * Conventions are those of msexpert.h: plain device pointers, 0 (MS_OK) or an MS_E* code with
 * ms_last_error(), arguments checked before any device work. The entry point is an addition to
 * ABI version 3.
 *
 * Inputs, one row per board (global row R = row_begin + r keys every random draw, so a shard of
 * rows [a, b) called with row_begin = a computes what the same rows of the whole call compute):
 *   logits f32[n,A]        the learner's policy logits; may be NULL only when beta >= 1;
 *   mask u8[n,A]           nonzero at legal (hidden) cells; a row with no legal cell counts as all
 *                          legal, as in ms_sample_masked;
 *   best u8[n,A]           the `best` output of ms_expert_targets (read only for `agree`);
 *   expert_action i64[n]   its `action` output (read only where kind != MS_EXPERT_NONE);
 *   kind u8[n]             its `kind` output.
 * 1 <= A <= 3968 (the boards of msenv.h), 1 <= n < 2^31, row_begin >= 0; beta and explore in
 * [0, 1]; mode is MS_DAGGER_GREEDY or MS_DAGGER_SAMPLE.
 *
 * Per row, with u01 the 24-bit keyed uniform of ms_sample_masked and sm64 its splitmix64:
 *   u   the uniform legal action: bit for bit what ms_sample_masked returns on zero logits with the
 *       same (seed, counter, row_begin): key 0.f - logf(-logf(u01(seed, counter, R, i))), `>`, the
 *       lowest index wins ties;
 *   l   the learner's action. MS_DAGGER_SAMPLE: what ms_sample_masked(logits, ...) returns with
 *       seed sm64(seed ^ MS_DAGGER_C_LEARNER) and the same counter. MS_DAGGER_GREEDY: the
 *       lowest-index legal cell whose logit is maximal; a NaN logit compares below everything.
 *       In both modes, when no legal cell qualifies (greedy: no legal logit above -inf; sample:
 *       every legal key NaN), l is the lowest-index legal cell: whatever the logits hold, l is a
 *       legal cell in [0, A);
 *   cb = u01(sm64(seed ^ MS_DAGGER_C_BETA), counter, R, 0),
 *   ce = u01(sm64(seed ^ MS_DAGGER_C_EXPLORE), counter, R, 0).
 * The first rule that matches decides:
 *   1. ce < explore                 action = u,             source = MS_DAGGER_SRC_UNIFORM
 *   2. cb >= beta                   action = l,             source = MS_DAGGER_SRC_LEARNER
 *   3. kind != MS_EXPERT_NONE       action = expert_action, source = MS_DAGGER_SRC_EXPERT
 *   4. otherwise                    action = u,             source = MS_DAGGER_SRC_UNIFORM
 * so beta = 1, explore = 0 never reads logits and gives where(kind != 0, expert_action, u), and
 * beta = 0, explore = 0 plays the learner everywhere.
 *
 * Outputs (any but `action` may be NULL):
 *   action i64[n]          the move to play;
 *   source u8[n]           who chose it (MS_DAGGER_SRC_*);
 *   learner_action i64[n]  l, or -1 when logits is NULL;
 *   agree u8[n]            1 iff logits is not NULL, kind != MS_EXPERT_NONE and best[l] != 0: the
 *                          learner's agreement with the teacher, whoever ends up playing.
 */
#ifndef MSDAGGER_H
#define MSDAGGER_H

#include <stdint.h>

#include "msexpert.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MS_DAGGER_GREEDY 0
#define MS_DAGGER_SAMPLE 1

#define MS_DAGGER_SRC_UNIFORM 0
#define MS_DAGGER_SRC_EXPERT 1
#define MS_DAGGER_SRC_LEARNER 2

#define MS_DAGGER_MAX_CELLS 3968

/* domain separation of the three keyed streams (none is ms_dropout_masks') */
#define MS_DAGGER_C_LEARNER 0xA0761D6478BD642Full
#define MS_DAGGER_C_BETA 0xE7037ED1A0B428DBull
#define MS_DAGGER_C_EXPLORE 0x8EBC6AF09C88C6E3ull

/* Device pointers; asynchronous on `stream`. One launch, one wavefront per row. */
int ms_dagger_act(const float* logits, const uint8_t* mask, const uint8_t* best, const int64_t* expert_action,
                  const uint8_t* kind, int64_t n, int32_t A, int64_t row_begin, uint64_t seed, uint64_t counter,
                  float beta, float explore, int32_t mode, int64_t* action, uint8_t* source,
                  int64_t* learner_action, uint8_t* agree, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MSDAGGER_H */
