/*
 * mslookahead.h — C ABI of the two-guess lookahead of the exact-posterior player: on a board
 * where every move risks a mine, score the nearly-as-safe cells by what the click buys, and choose
 * the cell most likely to survive this guess and, where no safe move follows, the next one too.
 *
 * Conventions are those of msposterior.h: plain pointers, 0 (MS_OK) or an MS_E* code with
 * ms_last_error(), arguments checked before any device work (a refused call writes nothing). The
 * entry points are additions to ABI version 3.
 *
 * The rule. A board is a *guess board* when its posterior status is MS_AVOID_DECIDED, it has a
 * hidden cell, and pmin (the smallest prob over its hidden cells) is > 0.
 *   candidates   the hidden cells with prob <= pmin + margin (f64), ordered by (prob ascending,
 *                cell index ascending), the first K of them; candidate 0 is the greedy pick of
 *                msexpert.h.
 *   outcomes     for candidate c and v = 0 .. 8, S(c, v) is the board with c revealed as well and
 *                number[c] = v, analysed with the same mine count M (no flood fill for v = 0).
 *                Z_v is its `configs`. It counts where S(c, v) is MS_AVOID_DECIDED (then Z_v > 0).
 *   value        t(c, v) = 1 if S(c, v) has exactly M hidden cells (the click wins), else 1 if
 *                some hidden cell of S(c, v) has prob == 0.0 (a safe move follows), else
 *                1 - pmin'(c, v), the safety of its least dangerous cell.
 *   score        score(c) = (sum_v Z_v t(c, v)) / Z: ascending v over the outcomes that count, f64,
 *                one multiply and one add per term, never fused, one division at the end.
 *   scored       c is scored iff |sum_v Z_v - Z (1 - p_c)| <= MS_LOOKAHEAD_SCORED_RTOL Z (1 - p_c)
 *                (the same sum order; each product and difference rounded on its own). The outcomes
 *                partition the layouts without a mine on c, so the two sides differ only when a
 *                search ran out of budget. An unscored candidate is never chosen for its score.
 *   choice       the scored candidate of largest score; ties go to the earlier candidate (smaller
 *                prob, then lower index). No scored candidate: candidate 0.
 *
 * On the device the analysis runs in three steps: ms_lookahead_expand writes the boards S(c, v),
 * the caller runs ms_posterior_states or ms_posterior_states_grouped on those cap*K*9 rows with
 * `live2` as its `live`, and ms_lookahead_score applies the rule. Row (s*K + k)*9 + v of the
 * expanded arrays is outcome v of candidate k of slot s.
 */
#ifndef MSLOOKAHEAD_H
#define MSLOOKAHEAD_H

#include <stdint.h>

#include "msposterior.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MS_LOOKAHEAD_MAX_K 16
#define MS_LOOKAHEAD_OUTCOMES 9
#define MS_LOOKAHEAD_SCORED_RTOL 1e-9

/* Device pointers; asynchronous on `stream`; three launches, no atomics.
 * In:  status u8[n], prob f64[n,H*W]   a posterior result of the boards;
 *      revealed, number u8[n,H,W]      the boards, as ms_posterior_states takes them.
 * 1 <= n < 2^31, H*W <= MS_AVOID_MAX_CELLS, 1 <= K <= MS_LOOKAHEAD_MAX_K, 0 <= margin <= 1,
 * 1 <= cap and cap*K*9 < 2^31.
 * Out (all required):
 *   slot i32[n]            the guess boards get 0, 1, ... in ascending board order; -1 on every other
 *                          board and on the guess boards past the first `cap`;
 *   count i32[1]           the number of guess boards, those past `cap` included;
 *   cand i32[cap,K]        the candidates of each slot, -1 where there are fewer than K and on unused
 *                          slots;
 *   revealed2, number2 u8[cap*K*9,H,W]   the boards S(c, v); written on live rows only;
 *   live2 u8[cap*K*9]      1 where the row holds a board: a candidate, and v at most the number of
 *                          hidden neighbours of c (a larger v cannot occur). */
int ms_lookahead_expand(const uint8_t* status, const double* prob, const uint8_t* revealed, const uint8_t* number,
                        int64_t n, int32_t H, int32_t W, int32_t K, double margin, int64_t cap, int32_t* slot,
                        int32_t* count, int32_t* cand, uint8_t* revealed2, uint8_t* number2, uint8_t* live2,
                        void* stream);

/* Device pointers; asynchronous on `stream`; two launches.
 * In:  slot, cand            as ms_lookahead_expand wrote them;
 *      prob f64[n,H*W], configs f64[n]   the posterior result of the boards;
 *      status2 u8[R], prob2 f64[R,H*W], configs2 f64[R], revealed2 u8[R,H,W], R = cap*K*9: the
 *      posterior result of the expanded rows and their revealed planes (hidden = not revealed; read
 *      on decided rows only).
 * Out (all required):
 *   action i64[n]          the chosen cell; -1 on boards without a slot;
 *   score f64[cap,K]       NaN where the candidate is unscored or padding;
 *   n_scored i32[n]        scored candidates (0 on boards without a slot);
 *   changed u8[n]          1 iff the choice is not candidate 0. */
int ms_lookahead_score(const int32_t* slot, const int32_t* cand, const double* prob, const double* configs,
                       const uint8_t* status2, const double* prob2, const double* configs2,
                       const uint8_t* revealed2, int32_t mine_count, int64_t n, int32_t H, int32_t W, int32_t K,
                       int64_t cap, int64_t* action, double* score, int32_t* n_scored, uint8_t* changed,
                       void* stream);

/* The whole pipeline on the host: every pointer is a HOST pointer, the call is synchronous and
 * makes no HIP call. The outcome boards are analysed by the host solver of ms_posterior_host
 * (grouped != 0: of ms_posterior_host_grouped) at `budget` nodes per query (0 = unbounded); an
 * outcome no layout reproduces counts as absent, as on the device. Nodes are counted as on the
 * device, so with the device's budget both run the same searches; on a CPU with fused multiply-add
 * the solver's sums are then rounded as the device rounds them and every output is bitwise the
 * device's (elsewhere a score may differ in its last bits and a tie fall the other way). The
 * expanded boards are not returned. `configs` is read on guess boards only. */
int ms_lookahead_host(const uint8_t* status, const double* prob, const double* configs, const uint8_t* revealed,
                      const uint8_t* number, int32_t mine_count, int64_t n, int32_t H, int32_t W, int32_t K,
                      double margin, int64_t cap, int64_t budget, int32_t grouped, int32_t* slot, int32_t* count,
                      int32_t* cand, int64_t* action, double* score, int32_t* n_scored, uint8_t* changed);

#ifdef __cplusplus
}
#endif

#endif /* MSLOOKAHEAD_H */
