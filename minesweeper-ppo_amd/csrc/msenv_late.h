// Late-start resets: the kernels behind ms_set_late_start, in the reference's shared-generator
// mode (k_late) and the keyed mode (k_late_keyed). Internal to libmsenv.so.
#ifndef MSENV_LATE_H
#define MSENV_LATE_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "msenv_board.h"
#include "msenv_click.h"
#include "msenv_pcg.h"
#include "msenv_place.h"
#include "msenv_wave.h"

namespace {

// ---------------------------------------------------------------------------
// Late-start resets (VecMinesweeper._apply_late_start, env.py:416-466).
// The reference draws every late start from ONE generator shared by all envs, in
// env order, and each env consumes a data-dependent number of draws, so the envs
// form a sequential chain: one wave walks them in order (each board's clicks are
// still wave-parallel: placement + flood fill as in k_step). Only envs flagged in
// `need` (the step's dones; all envs on ms_reset) are visited.
// ---------------------------------------------------------------------------
struct LateCfg {
  double prob;
  int32_t min_hidden, max_hidden, max_attempts, max_extra_steps;
};

// The late-start generator of the keyed mode (MS_LATE_KEYED): a PCG64 state built from
// (late seed, GLOBAL env index, the env's own PCG64 state at the reset) by splitmix64.
// The env's own state advances every episode (each episode places its mines), so every
// reset of every env has its own stream, independent of the world size and of the order
// in which envs reset. oracle/ms_oracle.c (keyed_late_rng) restates it.
__device__ __forceinline__ Pcg keyed_late_pcg(uint64_t seed, uint64_t gidx, uint64_t st_hi, uint64_t st_lo) {
  Pcg L;
  L.hi = splitmix64(seed ^ splitmix64(gidx ^ 0x6C8E9CF570932BD5ull));
  L.lo = splitmix64(L.hi ^ st_lo);
  L.ihi = splitmix64(L.lo ^ st_hi);
  L.ilo = splitmix64(L.ihi ^ 0xA0761D6478BD642Full) | 1ull;
  L.has32 = 0u;
  L.uinteger = 0u;
  return L;
}

// An env's state as late_env reads it: its rows in lanes and its meta (wave-uniform). k_late
// loads the next env's state before running the current one, so the load round trip of a
// reset overlaps the previous reset's clicks instead of heading the serial chain.
struct LateState {
  uint64_t mine, rev;
  uint64_t st_hi, st_lo, inc_hi, inc_lo;
  uint32_t has32, uinteger, step_count, flags;
};

template <int H_, int W_>
__device__ __forceinline__ LateState late_load(const KParams& p, int64_t env, const Geo<H_, W_>& g, int lane) {
  const int NW = g.NW();
  const EnvMeta* mp = p.meta + env;
  LateState s;
  s.mine = load_row(p.mine_words + env * NW, g, lane);
  s.rev = load_row(p.rev_words + env * NW, g, lane);
  s.st_hi = rfl64(mp->st_hi);
  s.st_lo = rfl64(mp->st_lo);
  s.inc_hi = rfl64(mp->inc_hi);
  s.inc_lo = rfl64(mp->inc_lo);
  s.has32 = rfl(mp->has32);
  s.uinteger = rfl(mp->uinteger);
  s.step_count = rfl((uint32_t)mp->step_count);
  s.flags = rfl(mp->flags);
  return s;
}

// The late-start generator of the shared mode as a jump-ahead batch: lane i holds output i + 1 of
// the batch (and the state after it), computed from the batch's base state with the handle's
// jump table, so a draw is a readlane instead of a serial 128-bit PCG step (~45 scalar
// instructions) on the critical chain. The buffered half-word (has32 / uinteger) follows
// numpy's next_uint32 as in pcg_next32. lr_state() is the PCG64 state after the last consumed
// output. The keyed mode keeps a plain Pcg (one reset per wave: nothing to batch).
struct LateRng {
  Pcg base;           // state before the batch; inc, has32 / uinteger are the generator's own
  uint32_t xlo, xhi;  // lane i: output i + 1 of the batch
  uint64_t sh, sl;    // lane i: the state after it
  int used;           // outputs of the batch consumed (uniform)
};
__device__ __forceinline__ void lr_fill(LateRng& R, const uint64_t (&J)[4]) {
  const uint64_t ci_lo = J[3] * R.base.ilo;
  const uint64_t ci_hi = __umul64hi(J[3], R.base.ilo) + J[3] * R.base.ihi + J[2] * R.base.ilo;
  const Out o = jump_out(R.base.hi, R.base.lo, J[0], J[1], ci_hi, ci_lo);
  R.sh = o.sh;
  R.sl = o.sl;
  R.xlo = (uint32_t)o.x;
  R.xhi = (uint32_t)(o.x >> 32);
  R.used = 0;
}
__device__ __forceinline__ uint64_t lr_next64(LateRng& R, const uint64_t (&J)[4]) {
  if (R.used == kWave) {
    R.base.hi = readlane64(R.sh, kWave - 1);
    R.base.lo = readlane64(R.sl, kWave - 1);
    lr_fill(R, J);
  }
  const int u = R.used++;
  return ((uint64_t)readlane32(R.xhi, u) << 32) | readlane32(R.xlo, u);
}
__device__ __forceinline__ uint64_t lr_next64(Pcg& L, const uint64_t (&J)[4]) {
  (void)J;
  return pcg_next64(L);
}
__device__ __forceinline__ uint32_t lr_next32(LateRng& R, const uint64_t (&J)[4]) {
  if (R.base.has32) {
    R.base.has32 = 0;
    return R.base.uinteger;
  }
  const uint64_t x = lr_next64(R, J);
  R.base.has32 = 1;
  R.base.uinteger = (uint32_t)(x >> 32);
  return (uint32_t)x;
}
// random_bounded_uint64(0, j), numpy's buffered Lemire (as pcg_bounded)
__device__ __forceinline__ uint32_t lr_bounded(LateRng& R, const uint64_t (&J)[4], uint32_t j) {
  if (j == 0) return 0;
  const uint32_t excl = j + 1u;
  uint64_t m = (uint64_t)lr_next32(R, J) * excl;
  uint32_t left = (uint32_t)m;
  if (left < excl) {
    const uint32_t thr = (0xffffffffu - j) % excl;
    while (left < thr) {
      m = (uint64_t)lr_next32(R, J) * excl;
      left = (uint32_t)m;
    }
  }
  return (uint32_t)(m >> 32);
}
__device__ __forceinline__ uint32_t lr_bounded(Pcg& L, const uint64_t (&J)[4], uint32_t j) {
  (void)J;
  return pcg_bounded(L, j);
}
__device__ __forceinline__ Pcg lr_state(const LateRng& R) {
  Pcg P = R.base;
  if (R.used > 0) {
    P.hi = readlane64(R.sh, R.used - 1);
    P.lo = readlane64(R.sl, R.used - 1);
  }
  return P;
}

// MS_DIAG builds: k_late's cycle accounting (tools/late_diag.py), summed over the launch in dacc:
// [0] whole launch, [1] envs visited, [2] late starts, [3] envs without a late start (draw + stores
// + emit), [4] first clicks (placement included), [5] extra-click loops, [6] extra clicks,
// [7] of them flood fills, [8] flood iterations, [9] late envs' stores + emit, [10] attempts,
// [14] cycles of flood fills (dilation + list rebuild), [15] cycles of flood clicks before the fill
#ifdef MS_DIAG
#define LSTAMP(k)                                          \
  do {                                                     \
    if (dacc) {                                            \
      const uint64_t t_ = __builtin_amdgcn_s_memtime();    \
      dacc[(k)] += t_ - tl_;                               \
      tl_ = t_;                                            \
    }                                                      \
  } while (0)
#define LCOUNT(k, v)            \
  do {                          \
    if (dacc) dacc[(k)] += (v); \
  } while (0)
#else
#define LSTAMP(k) do { } while (0)
#define LCOUNT(k, v) do { } while (0)
#endif


template <int H_, int W_, class Rng>
__device__ __forceinline__ void late_env(const KParams& p, Rng& L, const LateCfg& lc, int64_t env,
                                         const LateState& st, const uint64_t (&J)[4], uint64_t* sR, uint64_t* sM,
                                         uint32_t* sTab, const Geo<H_, W_>& g, int lane, uint64_t* dacc = nullptr) {
  (void)dacc;
#ifdef MS_DIAG
  uint64_t tl_ = __builtin_amdgcn_s_memtime();
  LCOUNT(1, 1);
#endif
  bool late = false;
  const int H = g.H, A = g.A(), NW = g.NW();
  const uint64_t rowmask = g.rowmask();
  const int safe_total = A - p.K;
  EnvMeta* mp = p.meta + env;
  uint64_t* mwords = p.mine_words + env * NW;
  uint64_t* rwords = p.rev_words + env * NW;
  uint64_t mine = st.mine;
  uint64_t rev = st.rev;
  Pcg rng;
  rng.hi = st.st_hi;
  rng.lo = st.st_lo;
  rng.ihi = st.inc_hi;
  rng.ilo = st.inc_lo;
  rng.has32 = st.has32;
  rng.uinteger = st.uinteger;
  int32_t step_count = (int32_t)st.step_count;
  bool fc = (st.flags & 1u) != 0;
  // prob <= 0 short-circuits before the draw (env.py:421)
  if (lc.prob > 0.0 && (double)(lr_next64(L, J) >> 11) * 0x1.0p-53 < lc.prob) {
    late = true;
    LCOUNT(2, 1);
    bool success = false;
    for (int att = 0; att < lc.max_attempts && !success; ++att) {
      LCOUNT(10, 1);
      if (fc) {  // env.reset() (env.py:87-101): the env's own RNG continues
        mine = 0ull;
        rev = 0ull;
        fc = false;
        step_count = 0;
      }
      const int first = (int)lr_bounded(L, J, (uint32_t)(A - 1));
      bool done, mc = false;
      int oc;
      uint32_t nw, tr;
      board_click(rng, mine, rev, fc, first, p, J, sTab, sR, g, lane, done, oc, nw, tr, mc);
      step_count += 1;
      LSTAMP(4);
      if (done) continue;
      int target = lc.min_hidden + (int)lr_bounded(L, J, (uint32_t)(lc.max_hidden - lc.min_hidden));
      target = target < safe_total ? target : safe_total;
      target = target > 1 ? target : 1;
      int revealed = (int)tr;
      // The extra clicks hit safe unrevealed cells of a placed board (the candidates are
      // ~mine & ~revealed, flags are never set), so each is MinesweeperEnv.step's reveal branch
      // alone: the candidates number safe_total - revealed (no count reduction), a cell with
      // adjacent mines reveals just itself (no flood-fill fixpoint), and the step ends the
      // episode only by a win. The mines are fixed now: their zero-cell map is built once.
      const uint64_t Um = wave_shr1(mine) | wave_shl1(mine);
      const uint64_t zero = ~(Um | (Um << 1) | (Um >> 1) | (mine << 1) | (mine >> 1)) & rowmask;
      // Compile-time boards of <= 256 cells (<= 32 columns, <= 16 rows) keep the candidates
      // (np.flatnonzero order) as a list in lane registers, four cell indices per lane (byte j of
      // lane l = entry 4l + j): the k-th is one readlane, and a numbered cell leaves the list by a
      // one-entry shift; the list is rebuilt from the rows after a flood fill.
      constexpr bool kList = H_ && W_ && H_ <= 16 && W_ <= 32 && H_ * W_ <= 256;
      uint32_t lword = 0u;
      auto build_list = [&]() {
        uint8_t* lst = reinterpret_cast<uint8_t*>(sTab);
        const uint32_t b = (uint32_t)(~mine & ~rev & (lane < H ? rowmask : 0ull));
        const uint32_t i0 = row_excl_scan16((uint32_t)__popc(b));
        // every column at once (predicated byte stores; a clear-lowest-bit loop is a serial,
        // divergent chain of the lone wave): cell j of the row goes to i0 + (candidates before it)
#pragma unroll
        for (int j = 0; j < W_; ++j)
          if ((b >> j) & 1u) lst[i0 + (uint32_t)__popc(b & ((1u << j) - 1u))] = (uint8_t)(lane * W_ + j);
        wave_sync();
        lword = reinterpret_cast<const uint32_t*>(lst)[lane];
        wave_sync();
      };
      if constexpr (kList) build_list();
      for (int k = 0; k < lc.max_extra_steps; ++k) {
        if (safe_total - revealed <= target) {
          success = true;
          break;
        }
        const uint32_t cnt = (uint32_t)(safe_total - revealed);
#ifdef MS_DIAG
        const uint64_t ts_ = __builtin_amdgcn_s_memtime();
#endif
        const uint32_t kk = lr_bounded(L, J, cnt - 1u);  // rng.choice(flatnonzero(...)) (row-major)
        LCOUNT(6, 1);
        int src, col;
        if constexpr (kList) {
          const int cell = (int)((readlane32(lword, (int)(kk >> 2)) >> (8u * (kk & 3u))) & 0xffu);
          src = cell / W_;
          col = cell - src * W_;
        } else {
          const uint64_t cand = ~mine & ~rev & (lane < H ? rowmask : 0ull);
          const uint32_t pc = (uint32_t)__popcll(cand);
          const uint32_t before = wave_excl_scan(pc);
          const bool mine_lane = kk >= before && kk < before + pc;
          const uint64_t who = __ballot(mine_lane);
          src = __ffsll((unsigned long long)who) - 1;
          // the k-th candidate of the row by a popcount bisection (a clear-lowest-bit loop cost
          // ~2x the whole click: tools/late_diag.py)
          const int sel = (W_ && W_ <= 32) ? select_bit32((uint32_t)cand, kk - before) : select_bit64(cand, kk - before);
          col = (int)readlane32((uint32_t)(mine_lane ? sel : 0), src);
        }
        if (((readlane64(zero, src) >> col) & 1ull) == 0ull) {
          if (lane == src) rev |= 1ull << col;
          revealed += 1;
          if constexpr (kList) {  // entry kk leaves the list: the entries after it move down one
            const uint32_t nxt = dpp32<0x130>(lword);  // lane l <- lane l + 1 (wave_shl:1)
            const uint32_t shifted = (lword >> 8) | (nxt << 24);
            const int lk = (int)(kk >> 2);
            const uint32_t keep = lane < lk ? 0xffffffffu : (lane == lk ? (1u << (8u * (kk & 3u))) - 1u : 0u);
            lword = (lword & keep) | (shifted & ~keep);
          }
        } else {  // flood_fill_reveal (env_numba.py:17-77) from a zero cell, as board_click
#ifdef MS_DIAG
          const uint64_t tf_ = __builtin_amdgcn_s_memtime();
          LCOUNT(15, tf_ - ts_);
#endif
          const uint64_t allow = ~mine & ~rev & (lane < H ? rowmask : 0ull);
          uint64_t Fr = (lane == src) ? (1ull << col) : 0ull;
          LCOUNT(7, 1);
          while (true) {
            LCOUNT(8, 1);
            const uint64_t S = Fr & zero;
            const uint64_t Dh = S | (S << 1) | (S >> 1);
            const uint64_t Dv = Dh | wave_shr1(Dh) | wave_shl1(Dh);
            const uint64_t Fn = Fr | (Dv & allow);
            const bool changed = __ballot(Fn != Fr) != 0ull;
            Fr = Fn;
            if (!changed) break;
          }
          rev |= Fr;
          revealed += (int)wave_sum((uint32_t)__popcll(Fr));
          if constexpr (kList) build_list();
#ifdef MS_DIAG
          LCOUNT(14, __builtin_amdgcn_s_memtime() - tf_);
#endif
        }
        step_count += 1;
        done = revealed >= safe_total;  // a win (env.py:133-140)
        if (done) break;
      }
      if (!success && !done && safe_total - revealed <= target) success = true;
      LSTAMP(5);
    }
    if (!success) {  // fallback: leave the board fresh (env.py:465-466)
      mine = 0ull;
      rev = 0ull;
      fc = false;
      step_count = 0;
    }
  }
  if (!late) {  // no late start: board, meta and obs are what the step (or ms_reset) just wrote
    LSTAMP(3);
    return;
  }
  if (lane == 0) {
    mp->st_hi = rng.hi;
    mp->st_lo = rng.lo;
    mp->has32 = rng.has32;
    mp->uinteger = rng.uinteger;
    mp->step_count = step_count;
    mp->flags = fc ? 1u : 0u;
  }
  store_rows(mwords, mine, sR, g, lane);
  store_rows(rwords, rev, sR, g, lane);
  __syncthreads();
  if (p.obs || p.mask || p.codes) {
    stage_rows(sR, sM, rev, mine, g, lane);
    emit_obs(p.obs ? p.obs + env * 10 * A : nullptr, p.mask ? p.mask + env * A : nullptr,
             p.codes ? p.codes + env * A : nullptr, sR, sM, fc, g, lane, reinterpret_cast<uint8_t*>(sTab));
  }
  __syncthreads();
  LSTAMP(9);
}

__device__ __forceinline__ void load_jump(const uint64_t* jump, int lane, uint64_t (&J)[4]) {
  const ulonglong2* e = reinterpret_cast<const ulonglong2*>(jump + 4 * lane);
  const ulonglong2 a0 = e[0], a1 = e[1];
  J[0] = a0.x;
  J[1] = a0.y;
  J[2] = a1.x;
  J[3] = a1.y;
}

// MS_LATE_SHARED (the reference): one wave walks the envs in order with the shared generator.
template <int H_, int W_>
__global__ __launch_bounds__(64) void k_late(KParams p, Pcg* lstate, LateCfg lc, const uint8_t* need) {
  __shared__ uint64_t sR[kWave];
  __shared__ uint64_t sM[kWave + 2];
  __shared__ uint32_t sTab[(H_ && W_) ? H_ * W_ : kMaxH * kMaxW];
  const int lane = lane_id();
  const Geo<H_, W_> g(p.H, p.W);
  LateRng L;
  L.base.hi = lstate->hi;
  L.base.lo = lstate->lo;
  L.base.ihi = lstate->ihi;
  L.base.ilo = lstate->ilo;
  L.base.has32 = lstate->has32;
  L.base.uinteger = lstate->uinteger;
  uint64_t J[4];
  load_jump(p.jump, lane, J);
  lr_fill(L, J);
  // the flags of 64 envs per load and ballot (one dependent scalar load per env cost ~0.5 us each);
  // the next env's state is loaded before the current env runs
  int64_t base = -kWave;
  uint64_t todo = 0ull;
  auto next_env = [&]() -> int64_t {
    while (todo == 0ull) {
      base += kWave;
      if (base >= p.n) return -1;
      const int64_t e = base + lane;
      todo = __ballot(e < p.n && (!need || need[e]));
    }
    const int l = __ffsll((unsigned long long)todo) - 1;
    todo &= todo - 1ull;
    return base + l;
  };
  uint64_t* dacc = nullptr;
#ifdef MS_DIAG
  uint64_t dv[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (p.diag) dacc = dv;
  const uint64_t t_begin = __builtin_amdgcn_s_memtime();
#endif
  int64_t cur = next_env();
  LateState sc = {};
  if (cur >= 0) sc = late_load(p, cur, g, lane);
  while (cur >= 0) {
    const int64_t nxt = next_env();
    LateState sn = sc;
    if (nxt >= 0) sn = late_load(p, nxt, g, lane);
    late_env(p, L, lc, cur, sc, J, sR, sM, sTab, g, lane, dacc);
    cur = nxt;
    sc = sn;
  }
#ifdef MS_DIAG
  if (dacc) {
    dv[0] = __builtin_amdgcn_s_memtime() - t_begin;
    if (lane == 0)
      for (int k = 0; k < 16; ++k) p.diag[k] = dv[k];
  }
#endif
  const Pcg Lf = lr_state(L);
  if (lane == 0) {
    lstate->hi = Lf.hi;
    lstate->lo = Lf.lo;
    lstate->has32 = Lf.has32;
    lstate->uinteger = Lf.uinteger;
  }
}

// MS_LATE_KEYED: one wave per env, every resetting env at once, each with its own
// keyed generator (keyed_late_pcg).
template <int H_, int W_>
__global__ __launch_bounds__(64) void k_late_keyed(KParams p, LateCfg lc, uint64_t seed, int64_t env_begin,
                                                   const uint8_t* need) {
  __shared__ uint64_t sR[kWave];
  __shared__ uint64_t sM[kWave + 2];
  __shared__ uint32_t sTab[(H_ && W_) ? H_ * W_ : kMaxH * kMaxW];
  const int64_t env = blockIdx.x;
  if (need && !need[env]) return;  // (uniform: one wave per workgroup)
  const int lane = lane_id();
  const Geo<H_, W_> g(p.H, p.W);
  uint64_t J[4];
  load_jump(p.jump, lane, J);
  const EnvMeta* mp = p.meta + env;
  Pcg L = keyed_late_pcg(seed, (uint64_t)(env_begin + env), rfl64(mp->st_hi), rfl64(mp->st_lo));
  late_env(p, L, lc, env, late_load(p, env, g, lane), J, sR, sM, sTab, g, lane);
}

}  // namespace

#endif  // MSENV_LATE_H
