/*
 * mssym.h — C ABI of the board symmetries: the mirror images and rotations of an [H, W] board,
 * applied to the planes of labelled states (ms_sym_gather), to a batch of cell codes for an
 * ensembled forward (ms_sym_expand) and, undone, to the network's per-cell outputs (ms_sym_mean).
 *
 * Conventions are those of msexpert.h: plain pointers, any plane may be NULL, 0 (MS_OK) or an
 * MS_E* code with ms_last_error(), arguments checked before any device work, device calls
 * asynchronous on `stream`. The entry points are additions to ABI version 3.
 *
 * A group element g has three bits, applied in this order to an [H, W] plane X:
 *   bit 2  transpose (square boards only);  bit 0  reverse the rows;  bit 1  reverse the columns.
 * In numpy: X = X.T if g & 4; X = X[::-1] if g & 1; X = X[:, ::-1] if g & 2. T_g(X) is the result.
 * Valid g: 0..7 where H == W, 0..3 otherwise; G(H, W) is 8 or 4. The inverse of g < 4 is g; for
 * g >= 4 it swaps bits 0 and 1 (5 <-> 6; 4 and 7 are their own inverses). The cell map lives in
 * one function (minesweeper-ppo_amd/csrc/mssym_map.h) that every kernel and the host entry use.
 *
 * Limits: 1 <= H, W; A = H*W <= MS_AVOID_MAX_CELLS; 1 <= n < 2^31.
 */
#ifndef MSSYM_H
#define MSSYM_H

#include <stdint.h>

#include "mssolve.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, no HIP call: writes A entries with T_g(X).flat[i] == X.flat[map[i]]. MS_EINVAL for
 * an invalid g (g >= 4 where H != W included), a bad shape or a NULL map. */
int ms_sym_cell_map_host(int32_t H, int32_t W, int32_t g, int32_t* map);

/* One launch that gathers and transforms: output row i is T_{g[i]} of source row rows[i], and
 * kind_out[i] = kind[rows[i]].
 *   rows i64[n]  source rows; NULL is the identity and needs n == B_src.   g u8[n].
 *   sources: codes, mask, best u8[B_src, A] (a torch bool is one byte), labels f32[B_src, A]
 *   (moved as bits: NaN payloads and -0.0 survive), kind u8[B_src]; outputs: the same with n rows.
 * A plane whose input or output pointer is NULL is skipped. A row with rows[i] outside
 * [0, B_src) or an invalid g[i] reads nothing: its cells in every output plane are 0 and its kind
 * is 0 (no target). status u8[n] (optional) is 1 for such a row, 0 otherwise. Nothing is clamped. */
int ms_sym_gather(const int64_t* rows, const uint8_t* g, int64_t n, int32_t H, int32_t W, int64_t B_src,
                  const uint8_t* codes, const uint8_t* mask, const uint8_t* best, const float* labels,
                  const uint8_t* kind, uint8_t* codes_out, uint8_t* mask_out, uint8_t* best_out, float* labels_out,
                  uint8_t* kind_out, uint8_t* status, void* stream);

/* out u8[G, n, H, W]: out[g] = T_g(codes) for g < G. G is 1, 4 or 8 (8: square boards only). */
int ms_sym_expand(const uint8_t* codes, int64_t n, int32_t H, int32_t W, int32_t G, uint8_t* out, void* stream);

/* x f32[G, n, A]: x[g] is a per-cell quantity of the boards transformed by g. out f32[n, A]:
 * out[i, c] = (1/G) * sum over g of y_g, with y_g the entry of x[g, i] that belongs to the
 * original cell c (T_g undone). The sum is f32 in a fixed pairwise tree,
 * ((y0+y1)+(y2+y3)) + ((y4+y5)+(y6+y7)) for G = 8 and (y0+y1)+(y2+y3) for G = 4, in plain adds,
 * then one multiply by the exact 1/G: G equal terms give the term back exactly.
 * H = W = 1 is the per-board scalar case. G as for ms_sym_expand. */
int ms_sym_mean(const float* x, int64_t n, int32_t H, int32_t W, int32_t G, float* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MSSYM_H */
