// Lane-packed boards: several small boards per wave. The board-wide primitives, the packed
// placements, click, obs emitters, state load and write-back that k_step_packed and
// k_run_packed (csrc/msenv.hip) are made of. Internal to libmsenv.so.
#ifndef MSENV_PACKED_H
#define MSENV_PACKED_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/msenv.h"
#include "../../include/msenv_debug.h"
#include "msenv_board.h"
#include "msenv_pcg.h"
#include "msenv_place.h"
#include "msenv_wave.h"

namespace {

// ---------------------------------------------------------------------------
// ms_step, lane-packed: four boards per wave for small boards (H <= 16, A <= 128,
// 1 <= K <= 16; the 9x9x10 and 8x8x10 benchmark shapes). Board b of the wave lives
// in DPP row b (lanes 16b..16b+15); lane 16b+r holds row r as a W-bit mask. Vertical
// neighbours are row_shr/row_shl:1 with bound_ctrl, which stop at the board edge;
// board sums are row_ror adds; a board-wide predicate is the board's 16 bits of a
// wave ballot; and every per-board scalar (PCG64 state, click, step count) is a VGPR
// that is uniform across the board's 16 lanes. The 4 boards' obs are one contiguous
// 40*A-float span, written as full 1 KiB float4 wave stores from a per-cell plane-bit
// table in this wave's LDS (wave-local: no workgroup barrier). A 9x9 board fills 9 of
// 64 lanes in k_step; here 36 of 64, with a quarter of the waves.
// ---------------------------------------------------------------------------

template <int B>
__device__ __forceinline__ float ub2f(uint32_t w) {  // byte B of w as f32 (one v_cvt_f32_ubyteB)
  return (float)((w >> (8 * B)) & 0xffu);
}

// LPB = lanes per board (16: four boards per wave, 32: two). A board's rows live in the first
// 16 lanes of its group, so the DPP row ops stay inside one DPP row either way.
template <int LPB>
__device__ __forceinline__ int board_base(int lane) { return lane & (64 - LPB); }
// sum over the board's lanes, result in each of them (row_ror:8,4,2,1; + the other row for 32)
template <int LPB>
__device__ __forceinline__ uint32_t board_sum(uint32_t v, int lane) {
  v += dpp32<0x128>(v);
  v += dpp32<0x124>(v);
  v += dpp32<0x122>(v);
  v += dpp32<0x121>(v);
  if (LPB == 32) v += bperm(v, lane ^ 16);
  return v;
}
template <int LPB>
__device__ __forceinline__ bool board_any(bool v, int lane) {
  constexpr uint64_t M = LPB == 64 ? ~0ull : ((1ull << LPB) - 1ull);
  return ((__ballot(v) >> board_base<LPB>(lane)) & M) != 0ull;
}
template <int LPB>
__device__ __forceinline__ uint32_t board_read(uint32_t v, int lane, int r) {  // v of the board's lane r
  return bperm(v, board_base<LPB>(lane) | (r & 15));
}
template <int LPB>
__device__ __forceinline__ uint64_t board_read64(uint64_t v, int lane, int r) {
  return ((uint64_t)board_read<LPB>((uint32_t)(v >> 32), lane, r) << 32) | board_read<LPB>((uint32_t)v, lane, r);
}

// row r (bits r*W .. r*W+W-1) of a 128-bit cell set
template <int H_, int W_>
__device__ __forceinline__ uint32_t set_row(uint64_t s0, uint64_t s1, int r, const Geo<H_, W_>& g) {
  if (r >= g.H) return 0u;
  const int s = r * g.W;
  const uint64_t v = s >= 64 ? (s1 >> (s - 64)) : ((s0 >> s) | (s ? (s1 << (64 - s)) : 0ull));
  return (uint32_t)(v & g.rowmask());
}
__device__ __forceinline__ bool set_has(uint64_t s0, uint64_t s1, uint32_t c) {
  return (((c < 64u) ? s0 : s1) >> (c & 63u)) & 1ull;
}
__device__ __forceinline__ void set_add(uint64_t& s0, uint64_t& s1, uint32_t c) {
  const uint64_t bit = 1ull << (c & 63u);
  if (c < 64u) s0 |= bit;
  else s1 |= bit;
}

// Placement of one packed board (same draws and result as place_fixpoint). The <= 16
// PCG64 outputs come from one jump-ahead per lane (lane r: output r+1), and lane r owns
// Floyd iteration r: j_r = pop-K+r, t_r = bounded draw in [0, j_r]. Floyd inserts t_r
// unless it is already chosen, then j_r. Because the j are distinct and exceed every
// earlier choice, "t_i already chosen" has a closed form: t_i equals an earlier t_k (which
// is chosen either way), or equals j_k for the one k = t_i - (pop-K) < i whose own t_k
// collided. Lane i gets the first from the board's 16 t values (one LDS broadcast read)
// and resolves the second by following k (a bpermute per link; chains are short).
// Mine rows are built with LDS ORs. Returns false on a Lemire rejection, leaving rng
// untouched (the caller then runs place_serial_packed).
template <int H_, int W_, int LPB>
__device__ bool place_packed(Pcg& rng, uint32_t& mine_out, const Block& B, int K, const uint64_t (&J)[4],
                             uint32_t* sBuf, int lane, uint64_t* dg = nullptr) {
  const int r = lane & (LPB - 1);
  (void)dg;
#ifdef MS_DIAG
#define QSTAMP(k)                                          \
  do {                                                     \
    if (dg && r == 0) dg[(k)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define QSTAMP(k) do { } while (0)
#endif
  QSTAMP(15);
  const int pop = B.pop;
  const int z0 = (pop == K) ? 1 : 0;
  const int nF = K - z0;
  const int D = nF + (K - 1);
  const int h0 = rng.has32 ? 1 : 0;
  const int rem = D - h0;
  const int n_out = (rem + 1) >> 1;  // <= K <= 16
  const uint64_t ci_lo = J[3] * rng.ilo;
  const uint64_t ci_hi = __umul64hi(J[3], rng.ilo) + J[3] * rng.ihi + J[2] * rng.ilo;
  const Out o = jump_out(rng.hi, rng.lo, J[0], J[1], ci_hi, ci_lo);
  // Lemire rejection test of the board's draws; the exact test (a 32-bit remainder) runs only
  // in a wave where some leftover is below its bound + 1 (place_fixpoint)
  uint32_t lft[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, bnd[3] = {0u, 0u, 0u};
  if (h0 && D > 0) {
    bnd[2] = (nF > 0) ? (uint32_t)(pop - K + z0) : (uint32_t)(K - 1);
    lft[2] = (uint32_t)((uint64_t)rng.uinteger * (bnd[2] + 1u));
  }
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
    const int pidx = h0 + 2 * r + hf;
    if (r < n_out && pidx < D) {
      const uint32_t d = hf ? (uint32_t)(o.x >> 32) : (uint32_t)o.x;
      bnd[hf] = pidx < nF ? (uint32_t)(pop - K + z0 + pidx) : (uint32_t)(K - 1 - (pidx - nF));
      lft[hf] = (uint32_t)((uint64_t)d * (bnd[hf] + 1u));
    }
  }
  const bool maybe = lemire_maybe(lft[0], bnd[0]) || lemire_maybe(lft[1], bnd[1]) || lemire_maybe(lft[2], bnd[2]);
  if (__ballot(maybe) != 0ull) {
    const bool rej = lemire_rejects(lft[0], bnd[0]) || lemire_rejects(lft[1], bnd[1]) || lemire_rejects(lft[2], bnd[2]);
    if (board_any<LPB>(rej, lane)) return false;
  }
  QSTAMP(10);
  // lane r: Floyd iteration i = r (draw pidx = i - z0, from output (pidx - h0) / 2)
  const int jr = pop - K + r;
  const int pidx = r - z0;
  const int idx = pidx - h0;
  const uint32_t wl = board_read<LPB>((uint32_t)o.x, lane, (idx >> 1) & 15);
  const uint32_t wh = board_read<LPB>((uint32_t)(o.x >> 32), lane, (idx >> 1) & 15);
  uint32_t d = (idx & 1) ? wh : wl;
  if (h0 && pidx == 0) d = rng.uinteger;
  const uint32_t t = r >= K ? 0xffffffffu : (r >= z0 ? (uint32_t)(((uint64_t)d * (uint32_t)(jr + 1)) >> 32) : 0u);
  sBuf[lane] = t;
  wave_sync();
  const uint4* tb = reinterpret_cast<const uint4*>(sBuf + board_base<LPB>(lane));
  const uint4 q0 = tb[0], q1 = tb[1], q2 = tb[2], q3 = tb[3];
  const uint32_t tk[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                           q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
  bool dup = false;
#pragma unroll
  for (int k = 0; k < 15; ++k) dup |= (k < r) && tk[k] == t;
  QSTAMP(11);
  const int ks = (int)t - (pop - K);  // t == j_ks
  const bool kv = r < K && ks >= 0 && ks < r;
  bool col = dup;
  while (true) {
    // every lane of the board takes part: ds_bpermute returns 0 from an EXEC-disabled source
    const uint32_t col_ks = board_read<LPB>(col ? 1u : 0u, lane, ks);
    const bool nc = dup || (kv && col_ks != 0u);
    const bool changed = __ballot(nc != col) != 0ull;
    col = nc;
    if (!changed) break;
  }
  QSTAMP(12);
  const int cell = map_block<W_>(col ? jr : (int)t, B);
  wave_sync();
  sBuf[lane] = 0u;
  wave_sync();
  if (r < K) atomicOr(&sBuf[board_base<LPB>(lane) + cell / W_], 1u << (cell % W_));
  wave_sync();
  mine_out = r < H_ ? sBuf[lane] : 0u;
  wave_sync();
  if (n_out > 0) {
    const int lq = n_out - 1;
    rng.hi = board_read64<LPB>(o.sh, lane, lq);
    rng.lo = board_read64<LPB>(o.sl, lane, lq);
    rng.uinteger = board_read<LPB>((uint32_t)(o.x >> 32), lane, lq);
  }
  if (D > 0) rng.has32 = (uint32_t)(rem & 1);
  QSTAMP(13);
  return true;
}

// Serial reference-order placement of one packed board: each lane of the board runs
// the same draws on its copy of the board's state (the Lemire-rejection fallback).
template <int H_, int W_>
__device__ void place_serial_packed(Pcg& rng, uint32_t& mine_out, const Block& B, int K, const Geo<H_, W_>& g,
                                    int r) {
  uint64_t s0 = 0ull, s1 = 0ull;
  for (int j = B.pop - K; j < B.pop; ++j) {
    uint32_t c = (uint32_t)map_block<W_>((int)pcg_bounded(rng, (uint32_t)j), B);
    if (set_has(s0, s1, c)) c = (uint32_t)map_block<W_>(j, B);
    set_add(s0, s1, c);
  }
  for (int i = K - 1; i >= 1; --i) (void)pcg_bounded(rng, (uint32_t)i);  // shuffle draws
  mine_out = set_row(s0, s1, r, g);
}

// Placement of one packed 16x16 board for K <= 48 (same draws and result as place_fixpoint):
// lane r of the board owns Floyd iterations r, r + 16, r + 32 and computes PCG64 outputs
// r + 1, r + 17, r + 33 from its one jump entry (k = r + 1) in three chunks of 16 (a chunk's
// base state is lane 15's state of the previous one). The outputs' words go to the board's LDS
// scratch, so iteration i reads its draw by index; "t_i repeats an earlier t" is an atomicMin
// into the board's 256-entry table, the collision chain follows k = t_i - (pop - K) by
// ds_bpermute (place_fixpoint's closed form), and the mine rows are LDS ORs. Returns false on a
// Lemire rejection, leaving rng untouched (the caller then runs place_serial_packed_w).
// scr: the wave's scratch, [4 boards][A] table | [4][96] output words | [4][16] rows.
template <int H_, int W_>
__device__ bool place_packed3(Pcg& rng, uint32_t& mine_out, const Block& B, int K, const uint64_t (&J)[4],
                              uint32_t* scr, int lane) {
  constexpr int A = H_ * W_;
  static_assert(H_ <= 16 && A <= 256, "16 rows, 8-bit cells");
  const int r = lane & 15, bb = lane >> 4;
  uint32_t* tab = scr + bb * A;
  uint32_t* xw = scr + 4 * A + bb * 96;
  uint32_t* rows = scr + 4 * A + 4 * 96 + bb * 16;
  const int pop = B.pop;
  const int z0 = (pop == K) ? 1 : 0;
  const int nF = K - z0;
  const int D = nF + (K - 1);
  const int h0 = rng.has32 ? 1 : 0;
  const int rem = D - h0;
  const int n_out = (rem + 1) >> 1;  // <= K <= 48
  const uint64_t ci_lo = J[3] * rng.ilo;
  const uint64_t ci_hi = __umul64hi(J[3], rng.ilo) + J[3] * rng.ihi + J[2] * rng.ilo;
  Out o[3];
  o[0] = jump_out(rng.hi, rng.lo, J[0], J[1], ci_hi, ci_lo);
#pragma unroll
  for (int c = 1; c < 3; ++c)
    o[c] = jump_out(board_read64<16>(o[c - 1].sh, lane, 15), board_read64<16>(o[c - 1].sl, lane, 15), J[0], J[1],
                    ci_hi, ci_lo);
  // Lemire rejection test of every consumed draw (exact test only where a leftover is low)
  uint32_t lft[7], bnd[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    lft[k] = 0xffffffffu;
    bnd[k] = 0u;
  }
  if (h0 && D > 0) {
    bnd[6] = (nF > 0) ? (uint32_t)(pop - K + z0) : (uint32_t)(K - 1);
    lft[6] = (uint32_t)((uint64_t)rng.uinteger * (bnd[6] + 1u));
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int q = 16 * c + r + 1;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int pidx = h0 + 2 * (q - 1) + hf;
      if (q <= n_out && pidx < D) {
        const uint32_t d = hf ? (uint32_t)(o[c].x >> 32) : (uint32_t)o[c].x;
        bnd[2 * c + hf] = pidx < nF ? (uint32_t)(pop - K + z0 + pidx) : (uint32_t)(K - 1 - (pidx - nF));
        lft[2 * c + hf] = (uint32_t)((uint64_t)d * (bnd[2 * c + hf] + 1u));
      }
    }
  }
  bool maybe = false;
#pragma unroll
  for (int k = 0; k < 7; ++k) maybe |= lemire_maybe(lft[k], bnd[k]);
  if (__ballot(maybe) != 0ull) {
    bool rej = false;
#pragma unroll
    for (int k = 0; k < 7; ++k) rej |= lemire_rejects(lft[k], bnd[k]);
    if (board_any<16>(rej, lane)) return false;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    xw[32 * c + 2 * r] = (uint32_t)o[c].x;
    xw[32 * c + 2 * r + 1] = (uint32_t)(o[c].x >> 32);
  }
#pragma unroll
  for (int k = 0; k < A / 16; ++k) tab[16 * k + r] = 0xffffffffu;
  wave_sync();
  int t[3], jj[3];
  bool valid[3];
#pragma unroll
  for (int s2 = 0; s2 < 3; ++s2) {
    const int i = r + 16 * s2;
    valid[s2] = i < K;
    jj[s2] = pop - K + i;
    const int pidx = i - z0;
    const int idx = pidx - h0;  // word of the fresh outputs (output idx / 2, half idx & 1)
    uint32_t d = xw[idx < 0 ? 0 : (idx > 95 ? 95 : idx)];
    if (h0 && pidx == 0) d = rng.uinteger;
    t[s2] = (valid[s2] && i >= z0) ? (int)(((uint64_t)d * (uint32_t)(jj[s2] + 1)) >> 32) : 0;
    if (valid[s2]) atomicMin(&tab[t[s2]], (uint32_t)i);
  }
  wave_sync();
  bool dup[3], col[3], kv[3];
  int ks[3];
#pragma unroll
  for (int s2 = 0; s2 < 3; ++s2) {
    const int i = r + 16 * s2;
    dup[s2] = valid[s2] && tab[t[s2]] != (uint32_t)i;
    ks[s2] = t[s2] - (pop - K);  // t_i == j_ks
    kv[s2] = valid[s2] && ks[s2] >= 0 && ks[s2] < i;
    col[s2] = dup[s2];
  }
  while (true) {
    bool changed = false, nc[3];
#pragma unroll
    for (int s2 = 0; s2 < 3; ++s2) {
      // every lane of the board takes part: ds_bpermute returns 0 from an EXEC-disabled source
      const int src = ks[s2] & 15, sl = (ks[s2] >> 4) & 3;
      const uint32_t c0 = board_read<16>(col[0] ? 1u : 0u, lane, src);
      const uint32_t c1 = board_read<16>(col[1] ? 1u : 0u, lane, src);
      const uint32_t c2 = board_read<16>(col[2] ? 1u : 0u, lane, src);
      const uint32_t cs = sl == 0 ? c0 : (sl == 1 ? c1 : c2);
      nc[s2] = dup[s2] || (kv[s2] && cs != 0u);
      changed |= nc[s2] != col[s2];
    }
#pragma unroll
    for (int s2 = 0; s2 < 3; ++s2) col[s2] = nc[s2];
    if (__ballot(changed) == 0ull) break;
  }
  rows[r] = 0u;
  wave_sync();
#pragma unroll
  for (int s2 = 0; s2 < 3; ++s2)
    if (valid[s2]) {
      const int cell = map_block<W_>(col[s2] ? jj[s2] : t[s2], B);
      atomicOr(&rows[cell / W_], 1u << (cell % W_));
    }
  wave_sync();
  mine_out = r < H_ ? rows[r] : 0u;
  wave_sync();
  if (n_out > 0) {  // the state after the last consumed output (board-uniform chunk c, lane lr)
    const int lq = n_out - 1, c = lq >> 4, lr = lq & 15;
    const uint64_t sh = c == 0 ? o[0].sh : (c == 1 ? o[1].sh : o[2].sh);
    const uint64_t sl = c == 0 ? o[0].sl : (c == 1 ? o[1].sl : o[2].sl);
    const uint64_t x = c == 0 ? o[0].x : (c == 1 ? o[1].x : o[2].x);
    rng.hi = board_read64<16>(sh, lane, lr);
    rng.lo = board_read64<16>(sl, lane, lr);
    rng.uinteger = board_read<16>((uint32_t)(x >> 32), lane, lr);
  }
  if (D > 0) rng.has32 = (uint32_t)(rem & 1);
  return true;
}

// Serial reference-order placement of one packed board of up to 256 cells (the Lemire
// fallback of place_packed3): every lane of the board runs the same draws.
template <int H_, int W_>
__device__ void place_serial_packed_w(Pcg& rng, uint32_t& mine_out, const Block& B, int K, int r) {
  static_assert(64 % W_ == 0 && H_ * W_ <= 256, "rows inside one 64-bit word");
  uint64_t s0 = 0ull, s1 = 0ull, s2 = 0ull, s3 = 0ull;
  auto word = [&](uint32_t c) -> uint64_t& { return c < 64u ? s0 : (c < 128u ? s1 : (c < 192u ? s2 : s3)); };
  for (int j = B.pop - K; j < B.pop; ++j) {
    uint32_t c = (uint32_t)map_block<W_>((int)pcg_bounded(rng, (uint32_t)j), B);
    if ((word(c) >> (c & 63u)) & 1ull) c = (uint32_t)map_block<W_>(j, B);
    word(c) |= 1ull << (c & 63u);
  }
  for (int i = K - 1; i >= 1; --i) (void)pcg_bounded(rng, (uint32_t)i);  // shuffle draws
  const uint32_t c0 = (uint32_t)(r * W_);
  mine_out = r < H_ ? (uint32_t)((word(c0) >> (c0 & 63u)) & ((1ull << W_) - 1ull)) : 0u;
}

// 16x16 boards four to a wave (k_step_packed): 16 rows in a 16-lane DPP row, K <= 48
template <int H_, int W_>
constexpr bool packable16() {
  return H_ == 16 && W_ == 16;
}

template <int H_, int W_>
constexpr bool packable() {
  // W_ <= 30: pk_emit's neighbour count shifts a u32 row by up to W_ + 1 bits
  return H_ >= 1 && H_ <= 16 && W_ >= 1 && W_ <= 30 && H_ * W_ <= 128;
}

// MS_DIAG builds: per-board phase stamps into this env's diag row (lane r == 0 of the board)
#ifdef MS_DIAG
#define DSTAMP(k)                                                            \
  do {                                                                       \
    if (dgs && r == 0) {                                                     \
      dgs[(k)] = __builtin_amdgcn_s_memtime();                               \
      if ((k) == 0) dgs[6] = __builtin_amdgcn_s_memrealtime();               \
      if ((k) == 5) dgs[7] = __builtin_amdgcn_s_memrealtime();               \
    }                                                                        \
  } while (0)
#else
#define DSTAMP(k) do { } while (0)
#endif

// LDS of one wave of the packed kernels
template <int H_, int W_, int BPW>
struct PackedLds {
  static constexpr int A = H_ * W_;
  static constexpr int IMG16 = (BPW * 10 * A + 15) / 16;  // 16-B units of the obs byte image
  uint4 img[IMG16];                     // the wave's boards' obs as 0/1 bytes, in store order
  uint32_t mask[(BPW * A + 3) / 4];     // their action-mask bytes
  alignas(16) uint32_t row[kWave];      // placement scratch; mine rows for the word store
  uint32_t rev[kWave];                  // revealed rows for the word store
};

// LDS of one wave of the 16x16 packed kernel: no byte image (pk_emit16 stores straight from
// the rows), the placement scratch of place_packed3, rows for the word store
template <int H_, int W_, int BPW>
struct PackedLds16 {
  static constexpr int A = H_ * W_;
  uint32_t scr[4 * (A + 96 + 16)];
  alignas(16) uint32_t row[kWave];
  uint32_t rev[kWave];
};

// One reveal on each board of the wave (env.py:103-137 minus the reward / step bookkeeping):
// first-click placement, mine hit, flood fill, win check. Per-board results are uniform
// across the board's lanes.
template <int H_, int W_, int LPB>
__device__ __forceinline__ void pk_click(const KParams& p, Pcg& rng, uint32_t& mine, uint32_t& rev, bool& fc, int cell,
                                         const uint64_t (&J)[4], uint32_t* sRow, int lane, uint64_t* dgs,
                                         bool& done, int& outcome, uint32_t& newly, uint32_t& total_rev,
                                         bool& mines_changed, bool& cell_rev) {
  constexpr int A = H_ * W_;
  constexpr uint32_t ROWMASK = (1u << W_) - 1u;
  const int r = lane & (LPB - 1);
  const Geo<H_, W_> g(H_, W_);
  const int ar = cell / W_, ac = cell - (cell / W_) * W_;
  done = false;
  outcome = MS_OUTCOME_NONE;
  newly = 0;
  cell_rev = board_any<LPB>(r == ar && ((rev >> ac) & 1u), lane);
  if (!cell_rev) {
    if (!fc) {
      const Block B = make_block<H_, W_>(cell, ar, ac, p.K, p.guarantee != 0);
      bool ok = false;
      if constexpr (packable16<H_, W_>()) {
        if (!(p.dbg_flags & MS_DBG_FORCE_SERIAL_PLACEMENT)) ok = place_packed3<H_, W_>(rng, mine, B, p.K, J, sRow, lane);
        if (!ok) place_serial_packed_w<H_, W_>(rng, mine, B, p.K, r);
      } else {
        if (!(p.dbg_flags & MS_DBG_FORCE_SERIAL_PLACEMENT)) ok = place_packed<H_, W_, LPB>(rng, mine, B, p.K, J, sRow, lane, dgs);
        if (!ok) place_serial_packed(rng, mine, B, p.K, g, r);
      }
      fc = true;
      mines_changed = true;
    }
    DSTAMP(2);
    const bool hit = board_any<LPB>(r == ar && ((mine >> ac) & 1u), lane);
    if (hit) {
      if (r == ar) rev |= 1u << ac;
      done = true;
      outcome = MS_OUTCOME_LOSS;
    } else {  // flood_fill_reveal (env_numba.py:17-77): dilation to a fixpoint inside the board's row
      const uint32_t U = row_shr1(mine) | row_shl1(mine);
      const uint32_t nb = U | (U << 1) | (U >> 1) | (mine << 1) | (mine >> 1);
      const uint32_t zero = ~nb & ROWMASK;
      const uint32_t allow = ~mine & ~rev & (r < H_ ? ROWMASK : 0u);
      uint32_t Fr = (r == ar) ? (1u << ac) : 0u;
      while (true) {
        const uint32_t S = Fr & zero;
        const uint32_t Dh = S | (S << 1) | (S >> 1);
        const uint32_t Dv = Dh | row_shr1(Dh) | row_shl1(Dh);
        const uint32_t Fn = Fr | (Dv & allow);
        const bool changed = __ballot(Fn != Fr) != 0ull;
        Fr = Fn;
        if (!changed) break;
      }
      rev |= Fr;
      newly = (uint32_t)__popc(Fr);
    }
  }
  const uint32_t packed = board_sum<LPB>(((uint32_t)__popc(rev) << 16) | newly, lane);
  total_rev = packed >> 16;
  newly = packed & 0xffffu;
  if (!cell_rev && outcome != MS_OUTCOME_LOSS && (int)total_rev >= A - p.K) {
    done = true;
    outcome = MS_OUTCOME_WIN;
  }
}

// Observation + action mask (env.py:172-196) of the wave's nbl live boards, written to the
// contiguous chunks ob (nbl*10*A floats, 16-B aligned) and mb (nbl*A bytes, 4-B aligned for
// BPW = 4, 2-B for BPW = 2). The obs are one-hot, so the wave zero-fills a byte image of them
// in LDS, each lane sets the (at most two) 1 bytes of each revealed cell of its row, and the
// wave copies the image out as whole 1 KiB float4 stores (4 bytes -> 4 floats with
// v_cvt_f32_ubyte0..3). OBS: the form of those stores (store_plane4; kObsStorePackedStep / Run).
template <int H_, int W_, int BPW, int LPB, int OBS>
__device__ __forceinline__ void pk_emit(float* ob, uint8_t* mb, int nbl, uint32_t mine, uint32_t rev, bool fc,
                                        PackedLds<H_, W_, BPW>& S, int lane, uint64_t* dgs) {
  constexpr int A = H_ * W_;
  constexpr int IMG16 = PackedLds<H_, W_, BPW>::IMG16;
  const int r = lane & (LPB - 1);
  uint8_t* sImg = reinterpret_cast<uint8_t*>(S.img);
  uint8_t* sMask = reinterpret_cast<uint8_t*>(S.mask);
#pragma unroll
  for (int k = 0; k < (IMG16 + kWave - 1) / kWave; ++k)
    if (k * kWave + lane < IMG16) S.img[k * kWave + lane] = make_uint4(0u, 0u, 0u, 0u);
  const uint32_t m1 = mine << 1;
  const uint32_t up1 = row_shr1(m1), dn1 = row_shl1(m1);  // rows r-1, r+1 (0 past the edge)
  wave_sync();
  if (r < H_) {
    uint8_t* img = sImg + (lane / LPB) * (10 * A) + r * W_;
    uint8_t* mk = sMask + (lane / LPB) * A + r * W_;
#pragma unroll
    for (int c = 0; c < W_; ++c) {
      const uint32_t cnt = (uint32_t)__popc((up1 >> c) & 7u) + (uint32_t)__popc((dn1 >> c) & 7u) +
                           ((m1 >> c) & 1u) + ((m1 >> (c + 2)) & 1u);
      const uint32_t rv = (rev >> c) & 1u;
      mk[c] = (uint8_t)(rv ^ 1u);
      // unconditional byte stores, no branch per cell: channel 0 = revealed, channel 1 + count
      // = 1 for a revealed cell after the first click (env.py:183-190); a hidden cell writes a
      // 0 over the zero-filled byte of its channel 1 + count
      img[c] = (uint8_t)rv;
      img[(1 + cnt) * A + c] = (uint8_t)(fc ? rv : 0u);
    }
  }
  DSTAMP(8);
  wave_sync();
  if (ob) {
    const uint32_t* s32 = reinterpret_cast<const uint32_t*>(sImg);
    if (nbl == BPW) {
      constexpr int NQ = BPW * 10 * A / 4;
      float4* o4 = reinterpret_cast<float4*>(ob);
#pragma unroll
      for (int k = 0; k < (NQ + kWave - 1) / kWave; ++k) {
        const int q = k * kWave + lane;
        if (q < NQ) {
          const uint32_t w = s32[q];
          store_plane4<OBS>(o4 + q, make_float4(ub2f<0>(w), ub2f<1>(w), ub2f<2>(w), ub2f<3>(w)));
        }
      }
    } else {  // partial last wave: whole float4s, then the odd tail floats
      const int nf = nbl * 10 * A;
      for (int q = lane; q < (nf >> 2); q += kWave) {
        const uint32_t w = s32[q];
        store_plane4<OBS>(reinterpret_cast<float4*>(ob) + q,
                          make_float4(ub2f<0>(w), ub2f<1>(w), ub2f<2>(w), ub2f<3>(w)));
      }
      for (int f = (nf & ~3) + lane; f < nf; f += kWave) store_plane1<OBS>(ob + f, (float)sImg[f]);
    }
  }
  DSTAMP(9);
  if (mb) {
    const int nbytes = nbl * A;
    if (BPW == 4) {
      for (int q = lane; q < (nbytes >> 2); q += kWave) reinterpret_cast<uint32_t*>(mb)[q] = S.mask[q];
      for (int i = (nbytes & ~3) + lane; i < nbytes; i += kWave) mb[i] = sMask[i];
    } else {
      const uint16_t* m16 = reinterpret_cast<const uint16_t*>(sMask);
      for (int q = lane; q < (nbytes >> 1); q += kWave) reinterpret_cast<uint16_t*>(mb)[q] = m16[q];
      if ((nbytes & 1) && lane == 0) mb[nbytes - 1] = sMask[nbytes - 1];
    }
  }
}

// Observation + action mask of the wave's nbl live 16x16 boards without an LDS image: per
// board, lane l covers row l / 4, cells 4 (l % 4) .. +3, fetching that row and its two
// neighbours from the board's lanes; each of the 10 channel planes is then one 1 KiB float4
// store of the wave and the mask one 256-B dword store. Same bytes as pk_emit (env.py:172-196).
template <int H_, int W_, int BPW>
__device__ __forceinline__ void pk_emit16(float* ob, uint8_t* mb, int nbl, uint32_t mine, uint32_t rev, bool fc,
                                          int lane) {
  static_assert(H_ == 16 && W_ == 16, "16x16 boards");
  constexpr int A = H_ * W_;
  const int row = lane >> 2, c0 = 4 * (lane & 3);
#pragma unroll
  for (int b = 0; b < BPW; ++b) {
    if (b >= nbl) break;  // (wave-uniform)
    const int src = 16 * b + row;
    const uint32_t m = bperm(mine, src), rv = bperm(rev, src);
    const uint32_t mu0 = bperm(mine, (src - 1) & 63), md0 = bperm(mine, (src + 1) & 63);
    const uint32_t mu = row > 0 ? mu0 : 0u, md = row < 15 ? md0 : 0u;
    const bool f = bperm(fc ? 1u : 0u, 16 * b) != 0u;
    const uint32_t m1 = m << 1, up1 = mu << 1, dn1 = md << 1;
    uint32_t cnt[4], rb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = c0 + e;
      cnt[e] = (uint32_t)__popc((up1 >> c) & 7u) + (uint32_t)__popc((dn1 >> c) & 7u) + ((m1 >> c) & 1u) +
               ((m1 >> (c + 2)) & 1u);
      rb[e] = (rv >> c) & 1u;
    }
    if (ob) {
      float4* o4 = reinterpret_cast<float4*>(ob + (size_t)b * 10 * A) + lane;
#pragma unroll
      for (int ch = 0; ch < 10; ++ch) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          v[e] = ch == 0 ? (float)rb[e] : ((f && rb[e] && cnt[e] + 1u == (uint32_t)ch) ? 1.f : 0.f);
        store_plane4(o4 + ch * (A / 4), make_float4(v[0], v[1], v[2], v[3]));
      }
    }
    if (mb)
      reinterpret_cast<uint32_t*>(mb + (size_t)b * A)[lane] =
          (rb[0] ^ 1u) | ((rb[1] ^ 1u) << 8) | ((rb[2] ^ 1u) << 16) | ((rb[3] ^ 1u) << 24);
  }
}

// EnvMeta and the row words of each live board (rows -> packed words through LDS)
template <int H_, int W_, int BPW, int LPB, class Lds>
__device__ __forceinline__ void pk_store_state(EnvMeta* mp, uint64_t* mwords, uint64_t* rwords, const Pcg& rng,
                                               int32_t step_count, bool fc, uint32_t mine, uint32_t rev,
                                               bool mines_changed, bool live, Lds& S, int lane) {
  constexpr int RPW = 64 / W_;
  constexpr int NW = (H_ + RPW - 1) / RPW;
  const int r = lane & (LPB - 1);
  store_meta(mp, rng, step_count, fc, live ? r : 1);
  const int rb = board_base<LPB>(lane);
  S.row[lane] = mine;
  S.rev[lane] = rev;
  wave_sync();
  if (live && r < NW) {
    uint64_t am = 0ull, ar_ = 0ull;
#pragma unroll
    for (int k = 0; k < RPW; ++k)
      if (r * RPW + k < H_) {
        am |= (uint64_t)S.row[rb + r * RPW + k] << (k * W_);
        ar_ |= (uint64_t)S.rev[rb + r * RPW + k] << (k * W_);
      }
    if (mines_changed) mwords[r] = am;
    rwords[r] = ar_;
  }
}

// Loads of one packed board: rows, this lane's jump entry (k = r+1: a placement uses outputs
// 1..K), and the meta (every lane of the board reads the same 48 B)
template <int H_, int W_>
__device__ __forceinline__ void pk_load(const EnvMeta* meta, const uint64_t* mine_words, const uint64_t* rev_words,
                                        const uint64_t* jump, int K, int64_t env, int r, uint32_t& mine, uint32_t& rev,
                                        uint64_t (&J)[4], Pcg& rng, int32_t& step_count, bool& fc) {
  constexpr int RPW = 64 / W_;
  constexpr int NW = (H_ + RPW - 1) / RPW;
  const Geo<H_, W_> g(H_, W_);
  const EnvMeta* mp = meta + env;
  mine = (uint32_t)load_row(mine_words + env * NW, g, r);
  rev = (uint32_t)load_row(rev_words + env * NW, g, r);
  J[0] = J[1] = J[2] = J[3] = 0ull;
  if (r < K) {
    const ulonglong2* e = reinterpret_cast<const ulonglong2*>(jump + 4 * r);
    const ulonglong2 a0 = e[0], a1 = e[1];
    J[0] = a0.x;
    J[1] = a0.y;
    J[2] = a1.x;
    J[3] = a1.y;
  }
  const ulonglong2 st = *reinterpret_cast<const ulonglong2*>(&mp->st_hi);
  const ulonglong2 inc = *reinterpret_cast<const ulonglong2*>(&mp->inc_hi);
  const uint4 m4 = *reinterpret_cast<const uint4*>(&mp->has32);
  rng.hi = st.x;
  rng.lo = st.y;
  rng.ihi = inc.x;
  rng.ilo = inc.y;
  rng.has32 = m4.x;
  rng.uinteger = m4.y;
  step_count = (int32_t)m4.z;
  fc = (m4.w & 1u) != 0;
}

}  // namespace

#endif  // MSENV_PACKED_H
