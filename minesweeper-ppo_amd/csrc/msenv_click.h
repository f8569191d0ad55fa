// One click on a one-board-per-wave board: what k_step, k_run (csrc/msenv.hip) and the
// late-start resets (csrc/msenv_late.h) share. Internal to libmsenv.so.
#ifndef MSENV_CLICK_H
#define MSENV_CLICK_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/msenv.h"
#include "../../include/msenv_debug.h"
#include "msenv_board.h"
#include "msenv_pcg.h"
#include "msenv_place.h"
#include "msenv_wave.h"

namespace {

// MS_DIAG builds: phase stamps of k_step into the env's diag row (board_click stamps slot 2
// when k_step passes it the env)
#ifdef MS_DIAG
#define STAMP(k)                                                             \
  do {                                                                        \
    if (p.diag && lane == 0) {                                                \
      p.diag[env * 16 + (k)] = __builtin_amdgcn_s_memtime();                  \
      if ((k) == 0) p.diag[env * 16 + 6] = __builtin_amdgcn_s_memrealtime();  \
      if ((k) == 5) p.diag[env * 16 + 7] = __builtin_amdgcn_s_memrealtime();  \
    }                                                                         \
  } while (0)
#else
#define STAMP(k) do { } while (0)
#endif

// ---------------------------------------------------------------------------
// One reveal on one board (MinesweeperEnv.step env.py:103-137 minus the reward /
// step bookkeeping): first-click placement, mine hit, flood fill, win check.
// Wave-uniform results: done, outcome, newly revealed, total revealed.
// ---------------------------------------------------------------------------
template <int H_, int W_>
__device__ __forceinline__ void board_click(Pcg& rng, uint64_t& mine, uint64_t& rev, bool& fc, int cell,
                                            const KParams& p, const uint64_t (&J)[4], uint32_t* sTab,
                                            uint64_t* sR, const Geo<H_, W_>& g, int lane, bool& done,
                                            int& outcome, uint32_t& newly, uint32_t& total_rev,
                                            bool& mines_changed, int64_t env = -1) {
  const int H = g.H, W = g.W, A = g.A();
  const uint64_t rowmask = g.rowmask();
  const int ar = cell / W, ac = cell - (cell / W) * W;
  done = false;
  outcome = MS_OUTCOME_NONE;
  newly = 0;
  const bool cell_rev = (readlane64(rev, ar) >> ac) & 1ull;
  if (!cell_rev) {
    if (!fc) {
      const Forbid F = make_forbid(cell, ar, ac, p.K, p.guarantee != 0, g);
      bool ok = false;
      if (!(p.dbg_flags & MS_DBG_FORCE_SERIAL_PLACEMENT)) {
        if (p.K >= 1 && p.K <= 128 && !(p.dbg_flags & MS_DBG_FORCE_CHAIN_PLACEMENT)) {
          Block B{};
          if constexpr (W_ > 3) B = make_block<H_, W_>(cell, ar, ac, p.K, p.guarantee != 0);
#ifdef MS_DIAG
          uint64_t* dgp = (p.diag && env >= 0) ? p.diag + env * 16 : nullptr;
#else
          uint64_t* dgp = nullptr;
#endif
          ok = p.K <= 64 ? place_fixpoint<H_, W_, 1>(rng, mine, F, B, p.K, J, sTab, sR, g, lane, dgp)
                         : place_fixpoint<H_, W_, 2>(rng, mine, F, B, p.K, J, sTab, sR, g, lane, dgp);
        }
        else
          ok = place_parallel(rng, mine, F, p.K, J, g, lane);
      }
      if (!ok) place_serial(rng, mine, F, p.K, g, lane);
      fc = true;
      mines_changed = true;
    }
    if (env >= 0) STAMP(2);
    const bool hit = (readlane64(mine, ar) >> ac) & 1ull;
    if (hit) {
      if (lane == ar) rev |= 1ull << ac;
      done = true;
      outcome = MS_OUTCOME_LOSS;
    } else {
      // ---- flood_fill_reveal (env_numba.py:17-77) as dilation to fixpoint ----
      const uint64_t U = wave_shr1(mine) | wave_shl1(mine);
      const uint64_t nb = U | (U << 1) | (U >> 1) | (mine << 1) | (mine >> 1);
      const uint64_t zero = ~nb & rowmask;
      const uint64_t allow = ~mine & ~rev & (lane < H ? rowmask : 0ull);
      uint64_t Fr = (lane == ar) ? (1ull << ac) : 0ull;
      while (true) {
        const uint64_t S = Fr & zero;
        const uint64_t Dh = S | (S << 1) | (S >> 1);
        const uint64_t Dv = Dh | wave_shr1(Dh) | wave_shl1(Dh);
        const uint64_t Fn = Fr | (Dv & allow);
        const bool changed = __ballot(Fn != Fr) != 0ull;
        Fr = Fn;
        if (!changed) break;
      }
      rev |= Fr;
      newly = (uint32_t)__popcll(Fr);
    }
  }
  // one reduction for both counts: total revealed (hi 16) | newly revealed (lo 16)
  const uint32_t packed = wave_sum(((uint32_t)__popcll(rev) << 16) | newly);
  total_rev = packed >> 16;
  newly = packed & 0xffffu;
  if (!cell_rev && outcome != MS_OUTCOME_LOSS && (int)total_rev >= A - p.K) {
    done = true;
    outcome = MS_OUTCOME_WIN;
  }
}

}  // namespace

#endif  // MSENV_CLICK_H
