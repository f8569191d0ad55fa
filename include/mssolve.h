/*
 * mssolve.h — C ABI of the avoidability analysis: for a board and the cell a policy is about
 * to reveal, is some hidden cell provably safe (the loss, if any, was avoidable), which cells,
 * and how large are the frontier's constraint components.
 *
 * Replaces analyze_avoidability (minesweeper/avoidability.py:145-394), which the reference's
 * evaluate_vec calls in Python once per env and step (eval.py:381-398). Conventions are those
 * of msenv.h: plain pointers, device arrays unless the comment says "host", asynchronous on
 * `stream`, any output may be NULL, 0 (MS_OK) or an MS_E* code with ms_last_error().
 *
 * The analysis (flags are never set, so hidden = not revealed):
 *   frontier    hidden cells with a revealed 8-neighbour;
 *   constraint  one per revealed non-mine cell with a frontier neighbour: its frontier
 *               neighbours hold exactly `adjacent count` mines;
 *   component   frontier cells linked through shared constraints (before any deduction);
 *   closure     unit rule (0 left: all safe; as many left as cells: all mines) and strict-
 *               subset rule (a within b: equal targets make b\a safe, a target difference of
 *               |b\a| makes b\a mines), to a fixpoint; if it proves a safe cell, that set is
 *               the answer (the reference returns here, no search);
 *   search      otherwise, per component over its still-free cells: a cell is safe iff "this
 *               cell is a mine" has no 0/1 assignment satisfying the component's constraints
 *               (complete depth-first search; the global mine count is not used).
 *
 * On the device every loop is bounded. The search counts one node per attempted value
 * assignment and stops a query at `budget` nodes; a board with a stopped query, with a
 * component of more than MS_AVOID_MAX_VARS free cells, or of more than MS_AVOID_MAX_CELLS cells
 * gets status MS_AVOID_UNDECIDED (never a guess). ms_avoid_host is the same analysis in plain
 * C++ without a budget: the exact fallback for undecided boards.
 */
#ifndef MSSOLVE_H
#define MSSOLVE_H

#include <stdint.h>

#include "msenv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status codes */
enum {
  MS_AVOID_SKIPPED = 0,   /* not analysed: not live, or before the first click; all outputs 0 */
  MS_AVOID_DECIDED = 1,
  MS_AVOID_UNDECIDED = 2  /* avoidable / n_safe / chosen_safe / safe_mask are 0, not an answer;
                             chosen_comp / n_comp / n_frontier / comp_size are valid unless the
                             board has more than MS_AVOID_MAX_CELLS cells (then 0 too) */
};

#define MS_AVOID_DEFAULT_BUDGET (1 << 18) /* nodes per query */
#define MS_AVOID_MAX_VARS 128             /* free cells of one component the device searches */
#define MS_AVOID_MAX_CELLS 512            /* cells of a board the device analyses */

/* Outputs, one entry per env ([n] unless noted):
 *   status u8, avoidable u8, n_safe i32 (number of provably safe cells), chosen_safe u8 (the
 *   chosen cell is one of them), chosen_comp i32 (size of the chosen cell's component; 1 for a
 *   hidden chosen cell on a board without frontier; 0 = None: not a frontier cell),
 *   n_comp i32, n_frontier i32 (= sum of the component sizes), safe_mask u8[n,H*W],
 *   max_nodes i32 (largest per-query node count; 0 if no search ran),
 *   comp_size i32[n,H*W] (size of the component a frontier cell belongs to, else 0).
 * chosen: int64[n], wrapped into [0, H*W) with Python `%` semantics like ms_step's actions.
 * live: u8[n] or NULL (= all); envs with live == 0 or before their first click get status 0. */

/* Analyses the handle's boards as they stand (before the step that `chosen` is for). Reads
 * only: board state, RNG streams and step counters are untouched. */
int ms_avoid(ms_handle* h, const int64_t* chosen, const uint8_t* live, uint8_t* status,
             uint8_t* avoidable, int32_t* n_safe, uint8_t* chosen_safe, int32_t* chosen_comp,
             int32_t* n_comp, int32_t* n_frontier, uint8_t* safe_mask, int32_t* max_nodes,
             int32_t* comp_size, void* stream);

/* The same analysis of boards given as arrays: revealed / mine u8[n,H,W] (nonzero = set),
 * first_click u8[n] (NULL = all done). H <= 64, W <= 62. budget: nodes per query, >= 1. */
int ms_avoid_states(const uint8_t* revealed, const uint8_t* mine, const uint8_t* first_click,
                    const int64_t* chosen, const uint8_t* live, int64_t n, int32_t H, int32_t W,
                    int32_t budget, uint8_t* status, uint8_t* avoidable, int32_t* n_safe,
                    uint8_t* chosen_safe, int32_t* chosen_comp, int32_t* n_comp,
                    int32_t* n_frontier, uint8_t* safe_mask, int32_t* max_nodes,
                    int32_t* comp_size, void* stream);

/* ms_avoid_states on the host: every pointer is a HOST pointer, the call is synchronous, there
 * is no budget and no size cap (status is 0 or 1), and no HIP call is made. Nodes are counted
 * as on the device, so max_nodes agrees wherever the device decides. */
int ms_avoid_host(const uint8_t* revealed, const uint8_t* mine, const uint8_t* first_click,
                  const int64_t* chosen, const uint8_t* live, int64_t n, int32_t H, int32_t W,
                  uint8_t* status, uint8_t* avoidable, int32_t* n_safe, uint8_t* chosen_safe,
                  int32_t* chosen_comp, int32_t* n_comp, int32_t* n_frontier, uint8_t* safe_mask,
                  int32_t* max_nodes, int32_t* comp_size);

/* Node budget per query for ms_avoid on this handle (default MS_AVOID_DEFAULT_BUDGET);
 * 1 <= nodes <= 2^30. */
int ms_avoid_set_budget(ms_handle* h, int32_t nodes);

#ifdef __cplusplus
}
#endif

#endif /* MSSOLVE_H */
