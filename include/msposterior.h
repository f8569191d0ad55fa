/*
 * msposterior.h — C ABI of the exact mine-probability posterior: for a board, the probability
 * that each hidden cell holds a mine given the revealed numbers and the mine count.
 *
 * Conventions are those of mssolve.h: plain pointers, device arrays unless the comment says
 * "host", asynchronous on `stream`, any output may be NULL, 0 (MS_OK) or an MS_E* code with
 * ms_last_error(). Arguments are checked before any device work.
 *
 * Definition (flags are never set, so hidden = not revealed). All layouts of exactly M mines on
 * hidden cells that reproduce every revealed number are equally likely; p(cell) is the share of
 * those layouts with a mine on the cell, `configs` their number. It is computed by components:
 *   frontier    hidden cells with a revealed 8-neighbour; one constraint per revealed cell;
 *   closure     the unit and strict-subset rules of mssolve.h to a fixpoint: cells proved safe
 *               have p = 0, cells proved mines have p = 1 and count towards M;
 *   components  the remaining free frontier cells, linked through constraints that still have
 *               free cells (the reduced system, after the closure);
 *   counts      per component j a complete depth-first search (variables in ascending cell
 *               order, value 0 before 1) counts N_j[k], the solutions with k mines, and for
 *               each of its cells v N_jv[k], those with a mine on v: one query per cell ("v is
 *               a mine") and one unconstrained query;
 *   combine     with U hidden cells that are neither frontier nor decided, R = M - closure
 *               mines, T the convolution of all N_j and O_j that of all but N_j:
 *                 Z = sum_s T[s] C(U, R-s)                                   (= configs)
 *                 p(v in j)   = sum_k sum_s N_jv[k] O_j[s] C(U, R-k-s) / Z
 *                 p(interior) = sum_s T[s] C(U-1, R-s-1) / Z
 * Counts are exact integers; the combination is f64 with sums in a fixed order. Every term is
 * non-negative and C(512, 256) ~ 5e152, so nothing cancels and nothing overflows on a board of
 * at most MS_AVOID_MAX_CELLS cells.
 *
 * On the device every loop is bounded. The search counts one node per attempted value
 * assignment and stops a query at `budget` nodes; a board with a stopped query, with a component
 * of more than MS_AVOID_MAX_VARS free cells, or of more than MS_AVOID_MAX_CELLS cells gets
 * status MS_AVOID_UNDECIDED (never a guess). An inconsistent board (Z = 0: no layout reproduces
 * the numbers) is MS_AVOID_UNDECIDED with zero outputs on the device and MS_EINVAL on the host.
 * msposterior_grouped.h declares the same analysis with the counts taken over groups of
 * equivalent cells, which finishes the weakly constrained components this search cannot.
 */
#ifndef MSPOSTERIOR_H
#define MSPOSTERIOR_H

#include <stdint.h>

#include "msenv.h"
#include "mssolve.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Nodes per query. Enumeration has a heavy tail: in evaluate_vec(RuleModel, 16x16x40, 4,096
 * episodes) 99.9 % of the 172,883 analysed boards need at most 2^13 nodes, 0.035 % need more than
 * 2^16 and 0.025 % more than 2^18 (weakly constrained components, whose solutions are too many to
 * list), and a board that runs out holds its launch for the whole budget (about 1.3 us per
 * node). 2^16 keeps 8x over the 99.9th percentile and 80x over the largest query of the
 * 16x16x40 fixture states (820), and bounds a launch at about 0.1 s. */
#define MS_POSTERIOR_DEFAULT_BUDGET (1 << 16)

/* Outputs, one entry per env:
 *   status u8[n]       MS_AVOID_SKIPPED (not live; before the first click on the handle path;
 *                      no revealed cell), MS_AVOID_DECIDED or MS_AVOID_UNDECIDED;
 *   prob f64[n,H*W]    0 at revealed cells, and 0 everywhere unless status is MS_AVOID_DECIDED;
 *   configs f64[n]     Z; 0 unless status is MS_AVOID_DECIDED;
 *   max_nodes i32[n]   largest per-query node count reached (0 if no search ran, or for an
 *                      inconsistent board).
 * live: u8[n] or NULL (= all). */

/* Analyses the handle's boards as they stand: M is the handle's mine count, the numbers are
 * recomputed from the mine rows. Reads only: board state, RNG streams and step counters are
 * untouched. */
int ms_posterior(ms_handle* h, const uint8_t* live, uint8_t* status, double* prob, double* configs,
                 int32_t* max_nodes, void* stream);

/* ms_posterior_labels, the same analysis written as training targets of the belief head, is
 * declared in msposterior_labels.h. */

/* The same analysis of boards given as arrays: revealed u8[n,H,W] (nonzero = set), number
 * u8[n,H,W] (adjacent mines; read at revealed cells only, so an observation is enough).
 * H <= 64, W <= 62, 0 <= mine_count <= H*W. budget: nodes per query, 1 <= budget <= 2^30. */
int ms_posterior_states(const uint8_t* revealed, const uint8_t* number, int32_t mine_count,
                        const uint8_t* live, int64_t n, int32_t H, int32_t W, int32_t budget,
                        uint8_t* status, double* prob, double* configs, int32_t* max_nodes,
                        void* stream);

/* ms_posterior_states on the host: every pointer is a HOST pointer, the call is synchronous, there
 * is no size cap and no HIP call is made. host_budget: nodes per query, 0 = unbounded; a board
 * with a stopped query is MS_AVOID_UNDECIDED. Nodes are counted as on the device, so max_nodes
 * and all integer counts agree wherever the device decides. An inconsistent board is MS_EINVAL. */
int ms_posterior_host(const uint8_t* revealed, const uint8_t* number, int32_t mine_count,
                      const uint8_t* live, int64_t n, int32_t H, int32_t W, int64_t host_budget,
                      uint8_t* status, double* prob, double* configs, int32_t* max_nodes);

/* Node budget per query for ms_posterior on this handle (default MS_POSTERIOR_DEFAULT_BUDGET);
 * 1 <= nodes <= 2^30. */
int ms_posterior_set_budget(ms_handle* h, int32_t nodes);

#ifdef __cplusplus
}
#endif

#endif /* MSPOSTERIOR_H */
