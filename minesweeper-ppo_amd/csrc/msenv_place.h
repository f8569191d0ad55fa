// First-click mine placement for one board per wave (csrc/msenv.hip board_click): the
// forbidden cells, numpy's choice() as Floyd's algorithm in reference draw order, and its
// three implementations -- serial, jump-ahead with a serial Floyd chain, and fully
// lane-parallel with a fixpoint over the collision chain. Internal to libmsenv.so.
#ifndef MSENV_PLACE_H
#define MSENV_PLACE_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "msenv_board.h"
#include "msenv_pcg.h"
#include "msenv_wave.h"

namespace {

// allowed-index -> cell for the ascending forbidden list f[0..m) (numpy's
// flatnonzero(~forbidden) order, env.py:302).
__device__ __forceinline__ int map_allowed(int t, const int (&f)[9], int m) {
#pragma unroll
  for (int i = 0; i < 9; ++i)
    if (i < m && f[i] <= t) ++t;
  return t;
}

// ---------------------------------------------------------------------------
// Mine placement (env.py:280-312): numpy's choice(allowed, K, replace=False)
// = Floyd over j in [pop-K, pop) + (K-1) discarded Fisher-Yates draws.
// ---------------------------------------------------------------------------
struct Forbid {  // ascending forbidden cells (the click's clipped 3x3 block, or the click)
  int f[9];
  int m;
  int pop;
};

template <int H_, int W_>
__device__ __forceinline__ Forbid make_forbid(int cell, int ar, int ac, int K, bool guarantee, const Geo<H_, W_>& g) {
  Forbid F;
  F.m = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) F.f[i] = 0;
  if (guarantee) {
#pragma unroll
    for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
      for (int dc = -1; dc <= 1; ++dc) {
        const int rr = ar + dr, cc = ac + dc;
        if (rr >= 0 && rr < g.H && cc >= 0 && cc < g.W) {  // row-major scan = ascending cells
#pragma unroll
          for (int i = 0; i < 9; ++i)
            if (i == F.m) F.f[i] = rr * g.W + cc;
          ++F.m;
        }
      }
  } else {
    F.f[0] = cell;
    F.m = 1;
  }
  F.pop = g.A() - F.m;
  if (F.pop < K) {  // env.py:303-307: relax to the clicked cell only
    F.f[0] = cell;
    F.m = 1;
    F.pop = g.A() - 1;
  }
  return F;
}

// One Floyd insertion in cell space; `mine` holds row r in lane r.
template <int H_, int W_>
__device__ __forceinline__ void floyd_insert(uint64_t& mine, int c1, int j, const Forbid& F, const Geo<H_, W_>& g,
                                             int lane) {
  int r1 = c1 / g.W;
  int col = c1 - r1 * g.W;
  if ((readlane64(mine, r1) >> col) & 1ull) {  // t already chosen: take j instead
    c1 = map_allowed(j, F.f, F.m);
    r1 = c1 / g.W;
    col = c1 - r1 * g.W;
  }
  if (lane == r1) mine |= 1ull << col;
}

// The forbidden cells of a placement (env.py:280-307) as a block: nr rows of nc cells from
// cell base0 (the click's clipped 3x3 neighbourhood, or the click alone: nr = nc = 1).
struct Block {
  int base0, nr, nc, pop;
};
template <int H_, int W_>
__device__ __forceinline__ Block make_block(int cell, int ar, int ac, int K, bool guarantee) {
  Block B;
  if (guarantee) {
    const int r0 = ar > 0 ? ar - 1 : 0, r1 = ar < H_ - 1 ? ar + 1 : H_ - 1;
    const int c0 = ac > 0 ? ac - 1 : 0, c1 = ac < W_ - 1 ? ac + 1 : W_ - 1;
    B.base0 = r0 * W_ + c0;
    B.nr = r1 - r0 + 1;
    B.nc = c1 - c0 + 1;
  } else {
    B.base0 = cell;
    B.nr = B.nc = 1;
  }
  B.pop = H_ * W_ - B.nr * B.nc;
  if (B.pop < K) {  // env.py:303-307: relax to the clicked cell only
    B.base0 = cell;
    B.nr = B.nc = 1;
    B.pop = H_ * W_ - 1;
  }
  return B;
}
// allowed index t -> cell (numpy's flatnonzero(~forbidden)[t], env.py:302), closed form:
// past base0 the allowed cells come in gaps of W - nc between the block's row runs.
template <int W_>
__device__ __forceinline__ int map_block(int t, const Block& B) {
  static_assert(W_ > 3, "a 3-wide block must leave a gap in every row");
  if (t < B.base0) return t;
  const int tp = t - B.base0;
  const int q = B.nc == 3 ? tp / (W_ - 3) : (B.nc == 2 ? tp / (W_ - 2) : tp / (W_ - 1));
  return B.base0 + tp + B.nc * (1 + (q < B.nr - 1 ? q : B.nr - 1));
}

// Serial reference-order placement (also the fallback of the parallel one).
template <int H_, int W_>
__device__ void place_serial(Pcg& rng, uint64_t& mine, const Forbid& F, int K, const Geo<H_, W_>& g, int lane) {
  mine = 0ull;
  for (int j = F.pop - K; j < F.pop; ++j) {
    const int t = (int)pcg_bounded(rng, (uint32_t)j);
    floyd_insert(mine, map_allowed(t, F.f, F.m), j, F, g, lane);
  }
  for (int i = K - 1; i >= 1; --i) (void)pcg_bounded(rng, (uint32_t)i);  // shuffle draws
}

__device__ __forceinline__ bool lemire_rejects(uint32_t left, uint32_t bound) {
  // numpy buffered_bounded_lemire_uint32: redraw iff leftover < (2^32-1-rng) % (rng+1)
  const uint32_t excl = bound + 1u;
  if (left >= excl) return false;
  return left < (0xffffffffu - bound) % excl;
}

// Parallel placement: the PCG64 outputs the placement consumes are computed
// lane-parallel by jump-ahead (state after k steps = A_k*s + C_k*inc, table
// `jt` for k = 1..64), every draw's Floyd value / Lemire test is evaluated in
// its lane, and only the set-membership chain of Floyd stays serial (one
// readlane test per draw). Returns false, leaving rng/mine untouched, if any
// consumed draw would be rejected by Lemire (p ~ 1e-6): the caller then runs
// place_serial, so results are always the reference's.
template <int H_, int W_>
__device__ bool place_parallel(Pcg& rng, uint64_t& mine_out, const Forbid& F, int K, const uint64_t (&J)[4],
                               const Geo<H_, W_>& g, int lane) {
  if (K == 0) {
    mine_out = 0ull;
    return true;
  }
  const int pop = F.pop;
  const int z0 = (pop == K) ? 1 : 0;  // Floyd j = 0 consumes no draw
  const int nF = K - z0;               // Floyd draws
  const int D = nF + (K - 1);          // + shuffle draws
  const int h0 = rng.has32 ? 1 : 0;    // draw 0 comes from the buffered half-word
  const int rem = D - h0;              // draws taken from fresh outputs (>= 0: D >= 1 when h0)
  const int n_out = (rem + 1) >> 1;
  uint64_t mine = 0ull;
  // Floyd iterations without a draw (only j = 0)
  for (int i = 0; i < z0; ++i) floyd_insert(mine, map_allowed(0, F.f, F.m), pop - K + i, F, g, lane);
  if (h0 && D > 0) {
    const uint32_t bound = (nF > 0) ? (uint32_t)(pop - K + z0) : (uint32_t)(K - 1);
    const uint64_t m64 = (uint64_t)rng.uinteger * (bound + 1u);
    if (lemire_rejects((uint32_t)m64, bound)) return false;
    if (nF > 0) floyd_insert(mine, map_allowed((int)(m64 >> 32), F.f, F.m), pop - K + z0, F, g, lane);
  }
  uint64_t bhi = rng.hi, blo = rng.lo;  // base state of the current chunk
  uint64_t fin_hi = rng.hi, fin_lo = rng.lo;
  uint32_t fin_uint = rng.uinteger;
  const uint64_t Ah = J[0], Al = J[1], Ch = J[2], Cl = J[3];
  // C_k * inc is the same for every chunk
  const uint64_t ci_lo = Cl * rng.ilo;
  const uint64_t ci_hi = __umul64hi(Cl, rng.ilo) + Cl * rng.ihi + Ch * rng.ilo;
  for (int c = 0; 64 * c < n_out; ++c) {
    const int q = 64 * c + lane + 1;  // this lane's output index (1-based)
    const uint64_t l1 = Al * blo;
    const uint64_t h1 = __umul64hi(Al, blo) + Al * bhi + Ah * blo;
    const uint64_t sl = l1 + ci_lo;
    const uint64_t sh = h1 + ci_hi + (sl < l1 ? 1ull : 0ull);
    const uint64_t v = sh ^ sl;
    const unsigned rot = (unsigned)(sh >> 58);
    const uint64_t x = (v >> rot) | (v << ((64u - rot) & 63u));
    int tc[2];
    bool rej = false;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int pidx = h0 + 2 * (q - 1) + hf;
      const uint32_t d = hf ? (uint32_t)(x >> 32) : (uint32_t)x;
      const bool is_floyd = pidx < nF;
      const uint32_t bound = is_floyd ? (uint32_t)(pop - K + z0 + pidx) : (uint32_t)(K - 1 - (pidx - nF));
      const uint64_t m64 = (uint64_t)d * (bound + 1u);
      if (q <= n_out && pidx < D) rej |= lemire_rejects((uint32_t)m64, bound);
      tc[hf] = is_floyd ? map_allowed((int)(m64 >> 32), F.f, F.m) : 0;
    }
    if (__ballot(rej) != 0ull) return false;
    // serial Floyd chain over this chunk's draws
    const int pbeg = h0 + 128 * c;
    const int pend = min(h0 + 128 * c + 128, nF);
    for (int pidx = pbeg; pidx < pend; ++pidx) {
      const int rel = pidx - pbeg;
      const int ln = rel >> 1;
      const int c1 = (rel & 1) ? (int)readlane32((uint32_t)tc[1], ln) : (int)readlane32((uint32_t)tc[0], ln);
      floyd_insert(mine, c1, pop - K + z0 + pidx, F, g, lane);
    }
    const int last = min(n_out - 64 * c, 64) - 1;  // lane holding this chunk's last output
    fin_hi = readlane64(sh, last);
    fin_lo = readlane64(sl, last);
    fin_uint = readlane32((uint32_t)(x >> 32), last);
    bhi = readlane64(sh, 63);
    blo = readlane64(sl, 63);
  }
  rng.hi = fin_hi;
  rng.lo = fin_lo;
  if (D > 0) {
    rng.has32 = (uint32_t)(rem & 1);
    rng.uinteger = fin_uint;
  }
  mine_out = mine;
  return true;
}

// x = XSL-RR(state after k steps from (bhi,blo)), jump entry of this lane (k = lane+1)
struct Out {
  uint64_t sh, sl, x;
};
__device__ __forceinline__ Out jump_out(uint64_t bhi, uint64_t blo, uint64_t Ah, uint64_t Al, uint64_t ci_hi,
                                        uint64_t ci_lo) {
  Out o;
  const uint64_t l1 = Al * blo;
  const uint64_t h1 = __umul64hi(Al, blo) + Al * bhi + Ah * blo;
  o.sl = l1 + ci_lo;
  o.sh = h1 + ci_hi + (o.sl < l1 ? 1ull : 0ull);
  const uint64_t v = o.sh ^ o.sl;
  const unsigned rot = (unsigned)(o.sh >> 58);
  o.x = (v >> rot) | (v << ((64u - rot) & 63u));
  return o;
}

// Fully lane-parallel placement for 1 <= K <= 128 (every benchmark board): the <= 128
// PCG64 outputs come from two jump-ahead chunks, and lane i (and i+64) owns Floyd iteration
// i: j_i = pop-K+i, t_i = its bounded draw in [0, j_i]. Floyd inserts t_i unless it is
// already chosen, then j_i. The j are distinct and larger than every earlier choice, so "t_i
// already chosen" has a closed form: t_i equals an earlier t_k (chosen either way: as itself
// or because it already was), or t_i equals j_k for the one k = t_i - (pop-K) < i whose own
// t_k collided. The first term is one LDS atomicMin per iteration into a table indexed by t
// (t_i repeats an earlier draw iff the table's minimum is not i); the second follows k by
// ds_bpermute until nothing changes (chains are short: 1-2 rounds). Returns false on a
// Lemire rejection (the caller falls back to place_serial), leaving rng untouched.
__device__ __forceinline__ bool lemire_maybe(uint32_t left, uint32_t bound) {  // a rejection is possible
  return left < bound + 1u;
}
// MS_DIAG builds: sub-phase stamps of a placement (diag slots 8..13 of the env)
#ifdef MS_DIAG
#define PSTAMP(k)                                                  \
  do {                                                             \
    if (dg && lane == 0) dg[(k)] = __builtin_amdgcn_s_memtime();    \
  } while (0)
#else
#define PSTAMP(k) do { } while (0)
#endif

// NS = iteration slots per lane: 1 for K <= 64 (one jump-ahead chunk), 2 for K <= 128.
// Compile-time shapes with W > 3 map allowed indices to cells in closed form (map_block).
template <int H_, int W_, int NS>
__device__ bool place_fixpoint(Pcg& rng, uint64_t& mine_out, const Forbid& F, const Block& B, int K,
                               const uint64_t (&J)[4], uint32_t* tab, uint64_t* srow, const Geo<H_, W_>& g, int lane,
                               uint64_t* dg = nullptr) {
  (void)B;
  (void)dg;
  PSTAMP(8);
  const int A = g.A(), W = g.W;
  const int pop = F.pop;
  const int z0 = (pop == K) ? 1 : 0;
  const int nF = K - z0;
  const int D = nF + (K - 1);
  const int h0 = rng.has32 ? 1 : 0;
  const int rem = D - h0;
  const int n_out = (rem + 1) >> 1;  // <= 128
  const uint64_t ci_lo = J[3] * rng.ilo;
  const uint64_t ci_hi = __umul64hi(J[3], rng.ilo) + J[3] * rng.ihi + J[2] * rng.ilo;
  const Out o0 = jump_out(rng.hi, rng.lo, J[0], J[1], ci_hi, ci_lo);
  Out o1 = o0;
  if (NS == 2 && n_out > 64) o1 = jump_out(readlane64(o0.sh, 63), readlane64(o0.sl, 63), J[0], J[1], ci_hi, ci_lo);
  PSTAMP(9);
  // Lemire rejection test of every consumed draw (draw p of output q, half hf). A draw can
  // only be rejected if its leftover is below bound + 1, which almost never happens: the
  // exact test (a 32-bit remainder) runs only in a wave where some draw is that low.
  uint32_t lft[5], bnd[5];
  bool maybe = false;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    lft[k] = 0xffffffffu;
    bnd[k] = 0u;
  }
  if (h0 && D > 0) {
    bnd[4] = (nF > 0) ? (uint32_t)(pop - K + z0) : (uint32_t)(K - 1);
    lft[4] = (uint32_t)((uint64_t)rng.uinteger * (bnd[4] + 1u));
  }
#pragma unroll
  for (int ch = 0; ch < NS; ++ch) {
    const uint64_t x = ch ? o1.x : o0.x;
    const int q = 64 * ch + lane + 1;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int pidx = h0 + 2 * (q - 1) + hf;
      if (q <= n_out && pidx < D) {
        const uint32_t d = hf ? (uint32_t)(x >> 32) : (uint32_t)x;
        bnd[2 * ch + hf] = pidx < nF ? (uint32_t)(pop - K + z0 + pidx) : (uint32_t)(K - 1 - (pidx - nF));
        lft[2 * ch + hf] = (uint32_t)((uint64_t)d * (bnd[2 * ch + hf] + 1u));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) maybe |= lemire_maybe(lft[k], bnd[k]);
  if (__ballot(maybe) != 0ull) {  // (uniform, rare) the exact test
    bool rej = false;
#pragma unroll
    for (int k = 0; k < 5; ++k) rej |= lemire_rejects(lft[k], bnd[k]);
    if (__ballot(rej) != 0ull) return false;
  }
  PSTAMP(10);
  // Floyd draws: lane owns iterations i = lane + 64 s
  int t[NS], jj[NS];
  bool valid[NS];
#pragma unroll
  for (int s2 = 0; s2 < NS; ++s2) {
    const int i = lane + 64 * s2;
    valid[s2] = i < K;
    jj[s2] = pop - K + i;
    const int pidx = i - z0;
    const int idx = pidx - h0;
    // ds_bpermute delivers the SOURCE lane's register: fetch both halves of both
    // chunks in converged control flow, then select by this lane's idx
    const int src = (idx >> 1) & 63;
    const uint32_t w0l = bperm((uint32_t)o0.x, src), w0h = bperm((uint32_t)(o0.x >> 32), src);
    uint32_t d = (idx & 1) ? w0h : w0l;
    if (NS == 2) {
      const uint32_t w1l = bperm((uint32_t)o1.x, src), w1h = bperm((uint32_t)(o1.x >> 32), src);
      if (idx >> 7) d = (idx & 1) ? w1h : w1l;
    }
    if (h0 && pidx == 0) d = rng.uinteger;
    t[s2] = (i >= z0) ? (int)(((uint64_t)d * (uint32_t)(jj[s2] + 1)) >> 32) : 0;
  }
  for (int c = lane; c < A; c += kWave) tab[c] = 0xffffffffu;
  wave_sync();
  PSTAMP(11);
#pragma unroll
  for (int s2 = 0; s2 < NS; ++s2)
    if (valid[s2]) atomicMin(&tab[t[s2]], (uint32_t)(lane + 64 * s2));
  wave_sync();
  bool dup[NS], col[NS], kv[NS];
  int ks[NS];
#pragma unroll
  for (int s2 = 0; s2 < NS; ++s2) {
    const int i = lane + 64 * s2;
    dup[s2] = valid[s2] && tab[t[s2]] != (uint32_t)i;
    ks[s2] = t[s2] - (pop - K);  // t_i == j_ks
    kv[s2] = valid[s2] && ks[s2] >= 0 && ks[s2] < i;
    col[s2] = dup[s2];
  }
  uint32_t rounds = 0;
  while (true) {
    ++rounds;
    bool changed = false;
    bool nc[NS];
#pragma unroll
    for (int s2 = 0; s2 < NS; ++s2) {
      // every lane takes part in the reads (ds_bpermute returns 0 from an EXEC-disabled lane)
      const int src = ks[s2] & 63;
      const uint32_t c0 = bperm(col[0] ? 1u : 0u, src);
      const uint32_t c1 = NS == 2 ? bperm(col[NS - 1] ? 1u : 0u, src) : 0u;
      nc[s2] = dup[s2] || (kv[s2] && ((ks[s2] >= 64 ? c1 : c0) != 0u));
      changed |= nc[s2] != col[s2];
    }
#pragma unroll
    for (int s2 = 0; s2 < NS; ++s2) col[s2] = nc[s2];
    if (__ballot(changed) == 0ull) break;
  }
#ifdef MS_DIAG
  if (dg && lane == 0) dg[14] = rounds;
#else
  (void)rounds;
#endif
  PSTAMP(12);
  srow[lane] = 0ull;
  wave_sync();
#pragma unroll
  for (int s2 = 0; s2 < NS; ++s2)
    if (valid[s2]) {
      int cell;
      if constexpr (W_ > 3) cell = map_block<W_>(col[s2] ? jj[s2] : t[s2], B);
      else cell = map_allowed(col[s2] ? jj[s2] : t[s2], F.f, F.m);
      const int r = cell / W;
      atomicOr((unsigned long long*)&srow[r], 1ull << (cell - r * W));
    }
  wave_sync();
  mine_out = lane < g.H ? srow[lane] : 0ull;
  wave_sync();
  // RNG state after the D draws
  if (n_out > 0) {
    const int lastq = n_out - 1;
    const Out& ol = (lastq >= 64) ? o1 : o0;
    rng.hi = readlane64(ol.sh, lastq & 63);
    rng.lo = readlane64(ol.sl, lastq & 63);
    rng.uinteger = readlane32((uint32_t)(ol.x >> 32), lastq & 63);
  }
  if (D > 0) rng.has32 = (uint32_t)(rem & 1);
  PSTAMP(13);
  return true;
}

}  // namespace

#endif  // MSENV_PLACE_H
