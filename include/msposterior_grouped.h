/*
 * msposterior_grouped.h — C ABI of the exact mine-probability posterior with the per-component
 * counting done over groups of equivalent cells. A second counting method beside msposterior.h's
 * enumerating one, opt-in: no entry point of msposterior.h or msposterior_labels.h changes. The
 * entry points are additions to ABI version 3; parameter lists, outputs and conventions are those
 * of their counterparts.
 *
 * Definition. Frontier, closure, consistency, components of the reduced system, U, R and the f64
 * combine are those of msposterior.h. Only the per-component counting differs:
 *   groups   within a component two free cells are equivalent when they belong to the same set
 *            of reduced constraints; a group is an equivalence class, its multiplicity n is
 *            1..8. Groups are numbered in ascending order of their smallest cell. A group has at
 *            most 8 constraints, like a cell; a constraint has at most 8 groups.
 *   search   depth-first over the groups in that order, a group taking the values 0 (first) to n:
 *            how many of its cells hold a mine. A value is pruned when, for one of the group's
 *            constraints, the assigned sum exceeds the target or the assigned sum plus the
 *            multiplicities of the groups still open falls short of it. One node is one attempted
 *            value of one group; the budget and max_nodes count these. A leaf with values v_g
 *            adds the weight prod_g C(n_g, v_g) (multiplied in ascending g) to N_j[sum_g v_g].
 *   queries  one unconstrained query, and one per group g: "the smallest cell of g is a mine".
 *            That cell is fixed before the search starts (it counts as one node, like the fixed
 *            variable of msposterior.h's query) and lowers the targets of g's constraints by one;
 *            g goes on with multiplicity n - 1 at its own place in the order and is passed over
 *            when n - 1 = 0. For a group of one cell this is msposterior.h's query. Every cell of
 *            g receives the query's result: the cells of a group are symmetric.
 *   counts   are f64: exact integers below 2^53; above that each addition rounds to nearest.
 *            Every term is non-negative, so nothing cancels, and the largest count, 2^128, is far
 *            from overflow.
 * Where the enumerating search decides, its counts are below 2^53 (it visits every solution), so
 * the grouped N_j[k] and N_jv[k] are the same integers; the combine runs on them in the same
 * order, so prob and configs are bitwise equal between the two methods on every board both
 * decide. The grouped search decides boards the enumerating one cannot: a weakly constrained
 * component has few groups however many solutions.
 *
 * Bounds are msposterior.h's: the budget (nodes per query), MS_AVOID_MAX_VARS free cells per
 * component, MS_AVOID_MAX_CELLS cells; a board past one of them, and on the device an
 * inconsistent board, is MS_AVOID_UNDECIDED with zero outputs. A component of at most
 * MS_AVOID_MAX_VARS free cells has at most that many groups, so there is no further cap on groups.
 */
#ifndef MSPOSTERIOR_GROUPED_H
#define MSPOSTERIOR_GROUPED_H

#include <stdint.h>

#include "msposterior.h"
#include "msposterior_labels.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest number of groups in a component the device analyses: MS_AVOID_MAX_VARS, so no cap of
 * its own (a component within the cell cap never has more groups than cells). */
#define MS_POSTERIOR_MAX_GROUPS 128

/* ms_posterior with grouped counting; reads the handle's ms_posterior_set_budget value. */
int ms_posterior_grouped(ms_handle* h, const uint8_t* live, uint8_t* status, double* prob,
                         double* configs, int32_t* max_nodes, void* stream);

/* ms_posterior_states with grouped counting. */
int ms_posterior_states_grouped(const uint8_t* revealed, const uint8_t* number, int32_t mine_count,
                                const uint8_t* live, int64_t n, int32_t H, int32_t W,
                                int32_t budget, uint8_t* status, double* prob, double* configs,
                                int32_t* max_nodes, void* stream);

/* ms_posterior_host with grouped counting: host pointers, synchronous, no size cap, no HIP call.
 * Nodes are counted as on the device, so max_nodes and all counts agree wherever the device
 * decides. */
int ms_posterior_host_grouped(const uint8_t* revealed, const uint8_t* number, int32_t mine_count,
                              const uint8_t* live, int64_t n, int32_t H, int32_t W,
                              int64_t host_budget, uint8_t* status, double* prob, double* configs,
                              int32_t* max_nodes);

/* ms_posterior_labels with grouped counting: the same outputs and `source` values. */
int ms_posterior_labels_grouped(ms_handle* h, int32_t budget, float* labels, uint8_t* valid,
                                uint8_t* source, int32_t* max_nodes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MSPOSTERIOR_GROUPED_H */
