// msenv.hip — MI355X (gfx950) vectorised Minesweeper board step + rollout kernels.
//
// Implements the board half of the C ABI of include/msenv.h (csrc/msrollout.hip has ms_gae,
// ms_sample_masked and ms_dropout_masks). Reference behaviour followed
// (yakvrz/minesweeper-ppo):
//   MinesweeperEnv.step            minesweeper/env.py:103-152
//   _place_mines_safe              minesweeper/env.py:280-312 (numpy choice, Floyd)
//   _compute_adjacent_counts       minesweeper/env.py:314-335
//   flood_fill_reveal              minesweeper/env_numba.py:17-77
//   _build_obs / action mask / aux minesweeper/env.py:163-196
//   VecMinesweeper init/reset/step minesweeper/env.py:382-511
//
// Design: one board per 64-lane wavefront, one wavefront per
// workgroup. Lane r holds row r of the board as a W-bit mask (W <= 62,
// H <= 64). The zero-region flood-fill is a frontier dilation to fixpoint:
// horizontal dilation by shifts inside the lane, vertical by cross-lane
// shuffles, termination by a wave ballot. The numpy-compatible PCG64 stream
// of each env is wave-uniform, so mine placement (Floyd's algorithm + the
// discarded shuffle draws) runs on scalar registers and builds the per-lane
// mine rows directly (membership test = one ballot). The f32 one-hot
// observation, which is ~97% of the bytes a step moves, is emitted as
// coalesced 16-B stores (one 1 KiB wave-instruction per channel plane on
// 16x16) from a per-cell code computed from LDS-staged rows.
//
// The device code is one translation unit cut into headers by concern:
//   msenv_wave.h    wave, DPP and bit primitives
//   msenv_pcg.h     numpy's PCG64, device and host; splitmix64
//   msenv_board.h   EnvMeta, KParams, geometry, row words, obs / aux / meta stores
//   msenv_place.h   first-click mine placement, one board per wave
//   msenv_click.h   board_click: one reveal on such a board
//   msenv_packed.h  several boards per wave: placement, click, emitters, state
//   msenv_tape.h    the synthetic tape policy (k_tape, tape_cell, pk_tape_cell)
//   msenv_late.h    late-start resets (k_late, k_late_keyed)
// This file holds the step and run kernels, reset / labels / snapshot / rng_state, the
// launchers and the C ABI.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <type_traits>
#include <vector>

#include "../../include/msenv.h"
#include "../../include/msenv_debug.h"
#include "msenv_internal.h"

#include "msenv_wave.h"
#include "msenv_pcg.h"
#include "msenv_board.h"
#include "msenv_place.h"
#include "msenv_click.h"
#include "msenv_packed.h"
#include "msenv_tape.h"
#include "msenv_late.h"

namespace {

// ---------------------------------------------------------------------------
// ms_step: one wave = one env.
// ---------------------------------------------------------------------------

// EPW boards per workgroup, one per wave, each with its own LDS slice: fewer,
// larger workgroups halve the dispatch cost of a 4096-board launch, and no
// wave ever waits on another (board code syncs with wave_sync only).
// The words the first loads need (p.meta, p.mine_words, p.rev_words, p.actions, p.jump, p.n,
// p.actions_i32, p.K) are passed again as leading flat arguments: 14 dwords, which the
// kernarg preload (Makefile, msenv.hip's rule) delivers in SGPRs at wave launch, so the
// prologue's loads issue without first waiting for an s_load of the by-value struct.
template <int H_, int W_, int EPW>
__global__ __launch_bounds__(64 * EPW) void k_step(EnvMeta* meta0, uint64_t* mine_words0, uint64_t* rev_words0,
                                                   const void* actions0, const uint64_t* jump0, int64_t n0,
                                                   int32_t actions_i32_0, int32_t K0, KParams p) {
  __shared__ uint64_t sR_all[EPW][kWave];
  __shared__ uint64_t sM_all[EPW][kWave + 2];
  __shared__ uint32_t sTab_all[EPW][(H_ && W_) ? H_ * W_ : kMaxH * kMaxW];
  const int lane = lane_id();
  const int wv = (EPW == 1) ? 0 : (int)rfl(threadIdx.x >> 6);
  // A wave past the last env (tail of the last workgroup) loads env n-1 and leaves
  // before any store: no early exit that would make every load wait for p.n.
  const int64_t env_raw = (int64_t)blockIdx.x * EPW + wv;
  const bool live = env_raw < n0;
  const int64_t env = live ? env_raw : n0 - 1;
  uint64_t* sR = sR_all[wv];
  uint64_t* sM = sM_all[wv];
  uint32_t* sTab = sTab_all[wv];
  STAMP(0);
  const KParamsWarm warm = kparams_warm(p);
  const Geo<H_, W_> g(p.H, p.W);
  const int A = g.A(), NW = g.NW();

  EnvMeta* mp = meta0 + env;
  uint64_t* mwords = mine_words0 + env * NW;
  uint64_t* rwords = rev_words0 + env * NW;
  // issue every load up front
  uint64_t mine = load_row(mwords, g, lane);
  uint64_t rev = load_row(rwords, g, lane);
  // jump-ahead entry k = lane+1 (2 KiB shared by every wave, L2-resident). Only a board
  // whose next click is its first needs it, but every wave loads it here, right behind
  // its rows: gating it on first_click_done would put a second dependent round trip on
  // exactly the placement waves that end the launch. A placement consumes at most
  // 2K-1 draws = K outputs, so only lanes < K need their entry.
  uint64_t J[4] = {0ull, 0ull, 0ull, 0ull};
  if (lane < K0) {
    const ulonglong2* e = reinterpret_cast<const ulonglong2*>(jump0 + 4 * lane);
    const ulonglong2 a0 = e[0], a1 = e[1];
    J[0] = a0.x;
    J[1] = a0.y;
    J[2] = a1.x;
    J[3] = a1.y;
  }
  Pcg rng;
  rng.hi = rfl64(mp->st_hi);
  rng.lo = rfl64(mp->st_lo);
  rng.ihi = rfl64(mp->inc_hi);
  rng.ilo = rfl64(mp->inc_lo);
  rng.has32 = rfl(mp->has32);
  rng.uinteger = rfl(mp->uinteger);
  int32_t step_count = (int32_t)rfl((uint32_t)mp->step_count);
  bool fc = (rfl(mp->flags) & 1u) != 0;
  // the action as two unconditional 4-B loads (int32: the element twice; int64: both
  // halves): no branch, so they issue right behind the meta loads
  const uint32_t* ap = reinterpret_cast<const uint32_t*>(actions0);
  const int64_t aw = actions_i32_0 ? env : 2 * env;
  const uint32_t a_lo = ap[aw], a_hi = ap[actions_i32_0 ? aw : aw + 1];
  int64_t a = actions_i32_0 ? (int64_t)(int32_t)a_lo : (int64_t)(((uint64_t)a_hi << 32) | a_lo);
  a = (int64_t)rfl64((uint64_t)a);
  int64_t cell64 = a % A;  // Python modulo (env.py:106)
  if (cell64 < 0) cell64 += A;
  const int cell = (int)cell64;
  kparams_warm_wait(warm);
  if (!live) return;
  STAMP(1);

  double reward = 0.0;
  bool done = false;
  int outcome = MS_OUTCOME_NONE;
  uint32_t newly = 0, total_rev = 0;
  bool mines_changed = false;
  board_click(rng, mine, rev, fc, cell, p, J, sTab, sR, g, lane, done, outcome, newly, total_rev, mines_changed,
              env);
  STAMP(3);
  if (outcome == MS_OUTCOME_LOSS) reward += p.loss_reward;
  if (outcome == MS_OUTCOME_WIN) reward += p.win_reward;
  reward -= p.step_penalty;
  step_count += 1;
  const int32_t step_out = step_count;  // reported before the auto-reset
  if (done) {  // auto-reset (env.py:497-498 -> reset env.py:87-101); RNG continues
    mine = 0ull;
    rev = 0ull;
    fc = false;
    step_count = 0;
    mines_changed = true;
  }
  STAMP(4);

  // ---- observation + action mask (env.py:172-196), issued before the state write-back:
  // the obs stores are ~97 % of the bytes and the launch ends when they drain ----
  if (p.obs || p.mask || p.codes) {
    stage_rows(sR, sM, rev, mine, g, lane);
    emit_obs(p.obs ? p.obs + env * 10 * A : nullptr, p.mask ? p.mask + env * A : nullptr,
             p.codes ? p.codes + env * A : nullptr, sR, sM, fc, g, lane, reinterpret_cast<uint8_t*>(sTab));
  }
  // the three aux stores go behind the obs burst, which does not need them
  store_aux(p, env, lane, reward, done, step_out, newly, total_rev, outcome, A);
  // ---- persist state ----
  store_meta(mp, rng, step_count, fc, lane);
  if (mines_changed) store_rows(mwords, mine, sR, g, lane);
  store_rows(rwords, rev, sR, g, lane);
  STAMP(5);
}

// ms_step on lane-packed boards (msenv_packed.h)
// (leading flat arguments as in k_step: the words the prologue's loads need, preloaded)
template <int H_, int W_, int WPG, int BPW>
__global__ __launch_bounds__(64 * WPG) void k_step_packed(EnvMeta* meta0, uint64_t* mine_words0, uint64_t* rev_words0,
                                                          const void* actions0, const uint64_t* jump0, int64_t n0,
                                                          int32_t actions_i32_0, int32_t K0, KParams p) {
  constexpr int LPB = kWave / BPW;  // lanes per board (the board's rows: its first H)
  constexpr bool BIG = packable16<H_, W_>();  // 16x16: place_packed3 + pk_emit16
  static_assert(BPW == 2 || BPW == 4, "boards per wave");
  static_assert(packable<H_, W_>() || (BIG && BPW == 4), "packed board shape");
  constexpr int A = H_ * W_;
  constexpr int RPW = 64 / W_;
  constexpr int NW = (H_ + RPW - 1) / RPW;
  using Lds = std::conditional_t<BIG, PackedLds16<H_, W_, BPW>, PackedLds<H_, W_, BPW>>;
  __shared__ Lds S_all[WPG];
  const int lane = lane_id();
  const int r = lane & (LPB - 1);
  const int wv = (WPG == 1) ? 0 : (int)rfl(threadIdx.x >> 6);
  Lds& S = S_all[wv];
  const int64_t env0 = ((int64_t)blockIdx.x * WPG + wv) * BPW;
  const bool wave_live = env0 < n0;
  const int64_t env_raw = env0 + (lane / LPB);
  const bool live = env_raw < n0;
  const int64_t env = live ? env_raw : n0 - 1;  // a board past the end loads env n-1, stores nothing
  uint64_t* dgs = (p.diag && live) ? p.diag + env * 16 : nullptr;
  (void)dgs;
  DSTAMP(0);
  uint32_t mine, rev;
  uint64_t J[4];
  Pcg rng;
  int32_t step_count;
  bool fc;
  pk_load<H_, W_>(meta0, mine_words0, rev_words0, jump0, K0, env, r, mine, rev, J, rng, step_count, fc);
  const uint32_t* ap = reinterpret_cast<const uint32_t*>(actions0);
  const int64_t aw = actions_i32_0 ? env : 2 * env;
  const uint32_t a_lo = ap[aw], a_hi = ap[actions_i32_0 ? aw : aw + 1];
  if (!wave_live) return;
  const int64_t a = actions_i32_0 ? (int64_t)(int32_t)a_lo : (int64_t)(((uint64_t)a_hi << 32) | a_lo);
  int64_t cell64 = a % A;  // Python modulo (env.py:106)
  if (cell64 < 0) cell64 += A;
  DSTAMP(1);
  bool done, mines_changed = false, cell_rev;
  int outcome;
  uint32_t newly, total_rev;
  uint32_t* scr;
  if constexpr (BIG) scr = S.scr;
  else scr = S.row;
  pk_click<H_, W_, LPB>(p, rng, mine, rev, fc, (int)cell64, J, scr, lane, dgs, done, outcome, newly, total_rev,
                        mines_changed, cell_rev);
  DSTAMP(3);
  double reward = 0.0;
  if (outcome == MS_OUTCOME_LOSS) reward += p.loss_reward;
  if (outcome == MS_OUTCOME_WIN) reward += p.win_reward;
  reward -= p.step_penalty;
  step_count += 1;
  store_aux(p, env, live ? r : kWave, reward, done, step_count, newly, total_rev, outcome, A);
  if (done) {  // auto-reset (env.py:497-498 -> reset env.py:87-101); RNG continues
    mine = 0u;
    rev = 0u;
    fc = false;
    step_count = 0;
    mines_changed = true;
  }
  DSTAMP(4);
  const int nbl = (n0 - env0 < BPW) ? (int)(n0 - env0) : BPW;  // live boards of this wave
  if constexpr (BIG) {
    if (p.obs || p.mask)
      pk_emit16<H_, W_, BPW>(p.obs ? p.obs + env0 * 10 * A : nullptr, p.mask ? p.mask + env0 * A : nullptr, nbl, mine,
                             rev, fc, lane);
    DSTAMP(9);
  } else {
    if (p.obs || p.mask)
      pk_emit<H_, W_, BPW, LPB, kObsStorePackedStep>(p.obs ? p.obs + env0 * 10 * A : nullptr,
                                                     p.mask ? p.mask + env0 * A : nullptr, nbl, mine, rev, fc, S, lane,
                                                     dgs);
  }
  pk_store_state<H_, W_, BPW, LPB>(meta0 + env, mine_words0 + env * NW, rev_words0 + env * NW, rng, step_count, fc,
                                   mine, rev, mines_changed, live, S, lane);
  DSTAMP(5);
}

// ---------------------------------------------------------------------------
// ms_reset: clear boards (RNG continues) + obs zeros + mask ones.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_reset(EnvMeta* meta, uint64_t* mw, uint64_t* rw, int64_t n,
                                                int NW, float* obs, uint8_t* mask, int A) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = tid; e < n; e += nthreads) {
    meta[e].step_count = 0;
    meta[e].flags = 0;
  }
  for (int64_t i = tid; i < n * NW; i += nthreads) {
    mw[i] = 0;
    rw[i] = 0;
  }
  if (obs) {
    const int64_t tot = n * 10 * (int64_t)A;
    if ((tot & 3) == 0) {
      float4* o4 = reinterpret_cast<float4*>(obs);
      for (int64_t i = tid; i < tot / 4; i += nthreads) store_plane4(o4 + i, make_float4(0.f, 0.f, 0.f, 0.f));
    } else {
      for (int64_t i = tid; i < tot; i += nthreads) store_plane1(obs + i, 0.f);
    }
  }
  if (mask)
    for (int64_t i = tid; i < n * (int64_t)A; i += nthreads) mask[i] = 1;
}

// ---------------------------------------------------------------------------
// ms_labels / ms_snapshot: one wave per env, cell-parallel.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_labels(const EnvMeta* meta, const uint64_t* mw, const uint64_t* rw,
                                               int64_t n, int H, int W, float* labels, uint8_t* valid) {
  __shared__ uint64_t sMine[kWave], sRev[kWave];
  const int lane = lane_id();
  const int64_t env = blockIdx.x;
  if (env >= n) return;
  const Geo<0, 0> g(H, W);
  const int NW = g.NW(), A = g.A();
  sMine[lane] = load_row(mw + env * NW, g, lane);
  sRev[lane] = load_row(rw + env * NW, g, lane);
  const bool fc = (meta[env].flags & 1u) != 0;
  __syncthreads();
  for (int i = lane; i < A; i += kWave) {
    const int r = i / W, c = i - r * W;
    const uint32_t mb = (uint32_t)(sMine[r] >> c) & 1u, rb = (uint32_t)(sRev[r] >> c) & 1u;
    if (labels) labels[env * A + i] = fc ? (float)mb : 0.f;
    if (valid) valid[env * A + i] = fc ? (uint8_t)(rb ^ 1u) : 0;
  }
}

__global__ __launch_bounds__(64) void k_snapshot(const EnvMeta* meta, const uint64_t* mw, const uint64_t* rw,
                                                 int64_t n, int H, int W, uint8_t* mine, uint8_t* revealed,
                                                 uint8_t* counts, uint8_t* first_click, int32_t* step_count) {
  __shared__ uint64_t sMine[kWave + 2], sRev[kWave];
  const int lane = lane_id();
  const int64_t env = blockIdx.x;
  if (env >= n) return;
  const Geo<0, 0> g(H, W);
  const int NW = g.NW(), A = g.A();
  const uint64_t m = load_row(mw + env * NW, g, lane);
  sRev[lane] = load_row(rw + env * NW, g, lane);
  sMine[lane + 1] = m << 1;
  if (lane == 0) {
    sMine[0] = 0;
    sMine[kWave + 1] = 0;
    if (first_click) first_click[env] = (uint8_t)(meta[env].flags & 1u);
    if (step_count) step_count[env] = meta[env].step_count;
  }
  __syncthreads();
  for (int i = lane; i < A; i += kWave) {
    const int r = i / W, c = i - r * W;
    if (mine) mine[env * A + i] = (uint8_t)((sMine[r + 1] >> (c + 1)) & 1ull);
    if (revealed) revealed[env * A + i] = (uint8_t)((sRev[r] >> c) & 1ull);
    if (counts) {
      const uint64_t up = sMine[r] >> c, mid = sMine[r + 1] >> c, dn = sMine[r + 2] >> c;
      counts[env * A + i] = (uint8_t)(__popcll(up & 7ull) + __popcll(dn & 7ull) + (mid & 1ull) + ((mid >> 2) & 1ull));
    }
  }
}

__global__ __launch_bounds__(256) void k_rng_state(const EnvMeta* meta, int64_t n, uint64_t* out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const EnvMeta m = meta[e];
  out[6 * e + 0] = m.st_hi;
  out[6 * e + 1] = m.st_lo;
  out[6 * e + 2] = m.inc_hi;
  out[6 * e + 3] = m.inc_lo;
  out[6 * e + 4] = m.has32;
  out[6 * e + 5] = m.uinteger;
}

// ---------------------------------------------------------------------------
// ms_run_tape: T consecutive (ms_tape_actions, ms_step) pairs in ONE launch.
// A wave keeps its board in registers (rows in lanes, the PCG64 state in SGPRs)
// for all T steps: per step it picks the tape action from the current board (the
// rule of k_tape, evaluated wave-parallel: DPP sums, an exclusive scan and a
// k-th-set-bit select), applies board_click, writes every output of the step,
// auto-resets, and goes on. Meta and rows are read once and written once. With no
// launch boundary between steps the waves drift apart, so one wave's obs stores
// overlap another's flood fill. Bit-exact with the two-call sequence.
// ---------------------------------------------------------------------------
struct RunParams {
  uint64_t t0;
  int32_t T, mode, slots;
  int64_t env_begin;
  int64_t* actions;  // optional: the action of each step
};

template <int H_, int W_, int EPW>
__global__ __launch_bounds__(64 * EPW) void k_run(KParams p, RunParams r) {
  __shared__ uint64_t sR_all[EPW][kWave];
  __shared__ uint64_t sM_all[EPW][kWave + 2];
  __shared__ uint32_t sTab_all[EPW][(H_ && W_) ? H_ * W_ : kMaxH * kMaxW];
  const int lane = lane_id();
  const int wv = (EPW == 1) ? 0 : (int)rfl(threadIdx.x >> 6);
  const int64_t env = (int64_t)blockIdx.x * EPW + wv;
  if (env >= p.n) return;
  uint64_t* sR = sR_all[wv];
  uint64_t* sM = sM_all[wv];
  uint32_t* sTab = sTab_all[wv];
  const Geo<H_, W_> g(p.H, p.W);
  const int A = g.A(), NW = g.NW();
  EnvMeta* mp = p.meta + env;
  uint64_t* mwords = p.mine_words + env * NW;
  uint64_t* rwords = p.rev_words + env * NW;
  uint64_t mine = load_row(mwords, g, lane);
  uint64_t rev = load_row(rwords, g, lane);
  uint64_t J[4] = {0ull, 0ull, 0ull, 0ull};
  if (lane < p.K) {
    const ulonglong2* e = reinterpret_cast<const ulonglong2*>(p.jump + 4 * lane);
    const ulonglong2 a0 = e[0], a1 = e[1];
    J[0] = a0.x;
    J[1] = a0.y;
    J[2] = a1.x;
    J[3] = a1.y;
  }
  Pcg rng;
  rng.hi = rfl64(mp->st_hi);
  rng.lo = rfl64(mp->st_lo);
  rng.ihi = rfl64(mp->inc_hi);
  rng.ilo = rfl64(mp->inc_lo);
  rng.has32 = rfl(mp->has32);
  rng.uinteger = rfl(mp->uinteger);
  int32_t step_count = (int32_t)rfl((uint32_t)mp->step_count);
  bool fc = (rfl(mp->flags) & 1u) != 0;
  const uint64_t gidx = (uint64_t)(r.env_begin + env);
  const int64_t n = p.n;
  for (int t = 0; t < r.T; ++t) {
    const int64_t slot = (r.slots ? (int64_t)t * n : 0) + env;
    const int cell = tape_cell(mine, rev, g, lane, gidx, r.t0 + (uint64_t)t, r.mode);
    double reward = 0.0;
    bool done = false;
    int outcome = MS_OUTCOME_NONE;
    uint32_t newly = 0, total_rev = 0;
    bool mines_changed = false;
    board_click(rng, mine, rev, fc, cell, p, J, sTab, sR, g, lane, done, outcome, newly, total_rev, mines_changed);
    if (outcome == MS_OUTCOME_LOSS) reward += p.loss_reward;
    if (outcome == MS_OUTCOME_WIN) reward += p.win_reward;
    reward -= p.step_penalty;
    step_count += 1;
    if (r.actions && lane == 0) r.actions[slot] = cell;
    store_aux(p, slot, lane, reward, done, step_count, newly, total_rev, outcome, A);
    if (done) {  // auto-reset; the RNG continues
      mine = 0ull;
      rev = 0ull;
      fc = false;
      step_count = 0;
    }
    if (p.obs || p.mask) {
      stage_rows(sR, sM, rev, mine, g, lane);
      emit_obs(p.obs ? p.obs + slot * 10 * A : nullptr, p.mask ? p.mask + slot * A : nullptr, nullptr, sR, sM, fc, g, lane,
               reinterpret_cast<uint8_t*>(sTab));
    }
    wave_sync();  // this step's LDS reads before the next step's placement / staging writes
  }
  store_meta(mp, rng, step_count, fc, lane);
  store_rows(mwords, mine, sR, g, lane);
  store_rows(rwords, rev, sR, g, lane);
}

// ms_run_tape on packed boards: k_run's T (tape, step) pairs per launch with k_step_packed's
// layout (four boards per wave). The synthetic policy's k-th valid cell is found per board
// (pk_tape_cell).
template <int H_, int W_, int WPG, int BPW>
__global__ __launch_bounds__(64 * WPG) void k_run_packed(KParams p, RunParams rp) {
  constexpr int LPB = kWave / BPW;
  constexpr bool BIG = packable16<H_, W_>();  // 16x16: place_packed3 + pk_emit16
  static_assert(BPW == 2 || BPW == 4, "boards per wave");
  static_assert(packable<H_, W_>() || (BIG && BPW == 4), "packed board shape");
  constexpr int A = H_ * W_;
  constexpr int RPW = 64 / W_;
  constexpr int NW = (H_ + RPW - 1) / RPW;
  using Lds = std::conditional_t<BIG, PackedLds16<H_, W_, BPW>, PackedLds<H_, W_, BPW>>;
  __shared__ Lds S_all[WPG];
  const int lane = lane_id();
  const int r = lane & (LPB - 1);
  const int wv = (WPG == 1) ? 0 : (int)rfl(threadIdx.x >> 6);
  Lds& S = S_all[wv];
  uint32_t* scr;
  if constexpr (BIG) scr = S.scr;
  else scr = S.row;
  const int64_t env0 = ((int64_t)blockIdx.x * WPG + wv) * BPW;
  if (env0 >= p.n) return;  // (wave-uniform)
  const int64_t env_raw = env0 + (lane / LPB);
  const bool live = env_raw < p.n;
  const int64_t env = live ? env_raw : p.n - 1;
  uint32_t mine, rev;
  uint64_t J[4];
  Pcg rng;
  int32_t step_count;
  bool fc;
  pk_load<H_, W_>(p.meta, p.mine_words, p.rev_words, p.jump, p.K, env, r, mine, rev, J, rng, step_count, fc);
  const uint64_t gidx = (uint64_t)(rp.env_begin + env);
  const int64_t n = p.n;
  const int nbl = (n - env0 < BPW) ? (int)(n - env0) : BPW;
  for (int t = 0; t < rp.T; ++t) {
    const int64_t sbase = rp.slots ? (int64_t)t * n : 0;
    const int cell = pk_tape_cell<H_, W_, LPB>(mine, rev, lane, gidx, rp.t0 + (uint64_t)t, rp.mode);
    bool done, mines_changed = false, cell_rev;
    int outcome;
    uint32_t newly, total_rev;
    pk_click<H_, W_, LPB>(p, rng, mine, rev, fc, cell, J, scr, lane, nullptr, done, outcome, newly, total_rev,
                          mines_changed, cell_rev);
    double reward = 0.0;
    if (outcome == MS_OUTCOME_LOSS) reward += p.loss_reward;
    if (outcome == MS_OUTCOME_WIN) reward += p.win_reward;
    reward -= p.step_penalty;
    step_count += 1;
    if (rp.actions && live && r == 0) rp.actions[sbase + env] = cell;
    store_aux(p, sbase + env, live ? r : kWave, reward, done, step_count, newly, total_rev, outcome, A);
    if (done) {  // auto-reset; the RNG continues
      mine = 0u;
      rev = 0u;
      fc = false;
      step_count = 0;
    }
    if constexpr (BIG) {
      if (p.obs || p.mask)
        pk_emit16<H_, W_, BPW>(p.obs ? p.obs + (sbase + env0) * 10 * A : nullptr,
                               p.mask ? p.mask + (sbase + env0) * A : nullptr, nbl, mine, rev, fc, lane);
    } else {
      if (p.obs || p.mask)
        pk_emit<H_, W_, BPW, LPB, kObsStorePackedRun>(p.obs ? p.obs + (sbase + env0) * 10 * A : nullptr,
                                                      p.mask ? p.mask + (sbase + env0) * A : nullptr, nbl, mine, rev,
                                                      fc, S, lane, nullptr);
    }
    wave_sync();  // this step's LDS reads before the next step's placement / image writes
  }
  pk_store_state<H_, W_, BPW, LPB>(p.meta + env, p.mine_words + env * NW, p.rev_words + env * NW, rng, step_count, fc,
                                   mine, rev, true, live, S, lane);
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
thread_local char g_err[512] = "";

int fail(int code, const char* fmt, const char* a = "", const char* b = "") {
  snprintf(g_err, sizeof g_err, fmt, a, b);
  return code;
}

int hip_fail(hipError_t e, const char* where) {
  return fail(MS_EHIP, "%s: %s", where, hipGetErrorString(e));
}

// the hipGetLastError tail of every launch
int launched(const char* where) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MS_OK : hip_fail(e, where);
}

}  // namespace

struct ms_handle {
  ms_cfg cfg;
  int64_t n_total, env_begin, n;
  int H, W, A, NW;
  int device;
  EnvMeta* meta;
  uint64_t* mine_words;
  uint64_t* rev_words;
  uint64_t* jump;  // [64][4] PCG64 jump-ahead table (device)
  uint64_t* diag;  // optional stamp buffer (MS_DIAG builds)
  uint32_t dbg_flags;
  int epw;         // boards per workgroup of k_step (4; generic shapes use 1)
  int late_on;     // ms_set_late_start called with prob > 0
  hipEvent_t ev_start, ev_stop;  // ms_set_timing_events (measurement only): stamp k_step / k_run
  LateCfg late;
  Pcg* late_rng;   // device: the shared late-start generator
  int late_mode;   // MS_LATE_SHARED (the reference's one generator) | MS_LATE_KEYED
  uint64_t late_seed;
  int32_t avoid_budget;  // ms_avoid_set_budget (mssolve.h); 0 = MS_AVOID_DEFAULT_BUDGET
  int32_t posterior_budget;  // ms_posterior_set_budget (msposterior.h); 0 = MS_POSTERIOR_DEFAULT_BUDGET
};

namespace {

bool shape_ok(const ms_cfg* c) {
  return c->H >= 1 && c->H <= kMaxH && c->W >= 1 && c->W <= kMaxW && c->mine_count >= 0 &&
         c->mine_count < c->H * c->W;
}

// The board shapes with kernels of their own; every other shape runs the generic <0, 0>
// instantiation. for_shape calls f with the list's entry that matches (H, W), as a value
// whose type carries the shape, or with Shape<0, 0>.
template <int H_, int W_>
struct Shape {
  static constexpr int H = H_, W = W_;
};
template <class... S>
struct Shapes {};
using StepShapes = Shapes<Shape<16, 16>, Shape<9, 9>, Shape<30, 16>, Shape<16, 30>, Shape<8, 8>>;  // and run
using TapeShapes = Shapes<Shape<16, 16>, Shape<9, 9>, Shape<30, 16>, Shape<16, 30>>;
using LateShapes = Shapes<Shape<16, 16>, Shape<9, 9>>;

template <class F>
void for_shape(Shapes<>, int, int, F&& f) {
  f(Shape<0, 0>{});
}
template <class S0, class... S, class F>
void for_shape(Shapes<S0, S...>, int H, int W, F&& f) {
  if (H == S0::H && W == S0::W) f(S0{});
  else for_shape(Shapes<S...>{}, H, W, f);
}

// 16x16 boards four to a wave from this many envs on: measured 2-4 % faster than the one-board
// kernel at 65,536, within +-3 % at 8,192-32,768 and 10 % slower at 4,096 (both store-bound at
// 32k+, the one-board kernel's 4x more waves hide latency better at 4k; profiles/r04/
// packed16_step.txt); MS_DBG_FORCE_PACKED takes the packed kernel at any count
constexpr int64_t kPack16MinEnvs = 65536;
// the multistep form (ms_run_tape), whose boards stay in registers across the launch's steps: the
// packed kernel measured 3 % faster at 4,096 envs, 3-12 % at 32,768 and ~10 % at 65,536 (a wash at
// 8,192; profiles/r04/packed16_run.txt), so it is taken at every env count
constexpr int64_t kPack16RunMinEnvs = 0;

// Whether the lane-packed kernels can take this launch: a shape they are built for, K within
// their placement's range, no debug flag that asks for another kernel, and obs / mask bases
// that their float4 / dword stores can use (16-B / 4-B aligned). 16x16 boards pack only from
// min_envs16 envs on (or with MS_DBG_FORCE_PACKED) and only four to a wave.
template <int H_, int W_>
bool packed_ok(const KParams& p, int64_t min_envs16) {
  const bool aligned = ((uintptr_t)p.obs & 15u) == 0 && ((uintptr_t)p.mask & 3u) == 0;
  const uint32_t other = MS_DBG_ONE_BOARD_PER_WAVE | MS_DBG_FORCE_CHAIN_PLACEMENT;
  if constexpr (packable16<H_, W_>())
    return p.K >= 1 && p.K <= 48 && !(p.dbg_flags & (other | MS_DBG_TWO_BOARDS_PER_WAVE)) &&
           (p.n >= min_envs16 || (p.dbg_flags & MS_DBG_FORCE_PACKED)) && aligned;
  else if constexpr (packable<H_, W_>())
    return p.K >= 1 && p.K <= 16 && !(p.dbg_flags & other) && aligned;
  else
    return false;
}

// boards per wave of a packed launch: four, or two for small boards under MS_DBG_TWO_BOARDS_PER_WAVE
template <int H_, int W_>
bool two_per_wave(const KParams& p) {
  return packable<H_, W_>() && (p.dbg_flags & MS_DBG_TWO_BOARDS_PER_WAVE);
}

constexpr int kPackedWPG = 4;  // waves per workgroup of the packed kernels
unsigned packed_grid(int64_t n, int bpw) {
  return (unsigned)((n + bpw * kPackedWPG - 1) / (bpw * kPackedWPG));
}

// ev0/ev1 non-null (ms_set_timing_events): the dispatch itself stamps the events, so their
// difference is the kernel's execution time as the profiler sees it (no launch gap)
struct Timed {
  hipStream_t s;
  hipEvent_t ev0, ev1;
};

// k_step / k_step_packed: the leading flat arguments (the words the kernarg preload delivers,
// in the order tests/test_kernargs_gpu.py pins), then the KParams block
template <class Kernel>
void launch_flat(Kernel k, unsigned grid, unsigned block, const Timed& t, const KParams& p) {
  hipExtLaunchKernelGGL(k, dim3(grid), dim3(block), 0, t.s, t.ev0, t.ev1, 0, p.meta, p.mine_words, p.rev_words,
                        p.actions, p.jump, p.n, p.actions_i32, p.K, p);
}

template <int H_, int W_>
void launch_step(const KParams& p, int epw, const Timed& t) {
  if constexpr (packable16<H_, W_>() || packable<H_, W_>()) {
    if (packed_ok<H_, W_>(p, kPack16MinEnvs) && !p.codes) {  // (the packed kernels write no codes)
      constexpr unsigned block = 64 * kPackedWPG;
      if constexpr (packable<H_, W_>()) {
        if (two_per_wave<H_, W_>(p))
          return launch_flat(k_step_packed<H_, W_, kPackedWPG, 2>, packed_grid(p.n, 2), block, t, p);
      }
      return launch_flat(k_step_packed<H_, W_, kPackedWPG, 4>, packed_grid(p.n, 4), block, t, p);
    }
  }
  // generic shapes keep one board per workgroup (their LDS table is sized for 64x62)
  if (H_ && W_ && epw == 4) launch_flat(k_step<H_, W_, 4>, (unsigned)((p.n + 3) / 4), 256, t, p);
  else launch_flat(k_step<H_, W_, 1>, (unsigned)p.n, 64, t, p);
}

template <int H_, int W_>
void launch_run(const KParams& p, const RunParams& r, const Timed& t) {
  if constexpr (packable16<H_, W_>() || packable<H_, W_>()) {
    // each step's 4-board obs / mask chunk must start 16-B / 4-B aligned, in every slot
    const bool slot_ok = !r.slots || ((p.n * H_ * W_) & 3) == 0;
    if (packed_ok<H_, W_>(p, kPack16RunMinEnvs) && slot_ok) {
      constexpr unsigned block = 64 * kPackedWPG;
      if constexpr (packable<H_, W_>()) {
        if (two_per_wave<H_, W_>(p)) {
          hipExtLaunchKernelGGL((k_run_packed<H_, W_, kPackedWPG, 2>), dim3(packed_grid(p.n, 2)), dim3(block), 0, t.s,
                                t.ev0, t.ev1, 0, p, r);
          return;
        }
      }
      hipExtLaunchKernelGGL((k_run_packed<H_, W_, kPackedWPG, 4>), dim3(packed_grid(p.n, 4)), dim3(block), 0, t.s,
                            t.ev0, t.ev1, 0, p, r);
      return;
    }
  }
  if (H_ && W_)
    hipExtLaunchKernelGGL((k_run<H_, W_, 4>), dim3((unsigned)((p.n + 3) / 4)), dim3(256), 0, t.s, t.ev0, t.ev1, 0, p, r);
  else hipExtLaunchKernelGGL((k_run<H_, W_, 1>), dim3((unsigned)p.n), dim3(64), 0, t.s, t.ev0, t.ev1, 0, p, r);
}

// The parameter block of a launch on h's boards, with the step's output buffers (any may be
// NULL). actions / actions_i32 / codes are the caller's to set.
KParams fill_params(const ms_handle* h, float* obs, uint8_t* mask, float* reward = nullptr, uint8_t* done = nullptr,
                    int32_t* step = nullptr, int32_t* last_new = nullptr, double* frac = nullptr,
                    int8_t* outcome = nullptr) {
  KParams p = {};
  p.obs = obs;
  p.mask = mask;
  p.reward = reward;
  p.done = done;
  p.step = step;
  p.last_new = last_new;
  p.frac = frac;
  p.outcome = outcome;
  p.meta = h->meta;
  p.mine_words = h->mine_words;
  p.rev_words = h->rev_words;
  p.n = h->n;
  p.H = h->H;
  p.W = h->W;
  p.K = h->cfg.mine_count;
  p.guarantee = h->cfg.guarantee_safe_neighborhood ? 1 : 0;
  p.win_reward = h->cfg.win_reward;
  p.loss_reward = h->cfg.loss_reward;
  p.step_penalty = h->cfg.step_penalty;
  p.jump = h->jump;
  p.diag = h->diag;
  p.dbg_flags = h->dbg_flags;
  return p;
}

int launch_late(const ms_handle* h, const KParams& p, const uint8_t* need, hipStream_t s) {
  for_shape(LateShapes{}, h->H, h->W, [&](auto sh) {
    using S = decltype(sh);
    if (h->late_mode == MS_LATE_KEYED)
      hipLaunchKernelGGL((k_late_keyed<S::H, S::W>), dim3((unsigned)p.n), dim3(64), 0, s, p, h->late, h->late_seed,
                         h->env_begin, need);
    else hipLaunchKernelGGL((k_late<S::H, S::W>), dim3(1), dim3(64), 0, s, p, h->late_rng, h->late, need);
  });
  return launched("late-start launch");
}

int do_step(ms_handle* h, const void* actions, int i32, float* obs, uint8_t* mask, float* reward,
            uint8_t* done, int32_t* step, int32_t* last_new, double* frac, int8_t* outcome, void* stream,
            uint8_t* codes = nullptr) {
  if (!h) return fail(MS_EINVAL, "ms_step: null handle");
  if (!actions) return fail(MS_EINVAL, "ms_step: null actions");
  if (codes && ((h->H * h->W) & 3) == 0 && ((uintptr_t)codes & 3u) != 0)
    return fail(MS_EINVAL, "ms_step_codes: codes must be 4-byte aligned");
  KParams p = fill_params(h, obs, mask, reward, done, step, last_new, frac, outcome);
  p.actions = actions;
  p.actions_i32 = i32;
  p.codes = codes;
  hipStream_t s = (hipStream_t)stream;
  if (h->late_on && !done) return fail(MS_EINVAL, "ms_step: late start needs the done output");
  for_shape(StepShapes{}, h->H, h->W, [&](auto sh) {
    using S = decltype(sh);
    launch_step<S::H, S::W>(p, h->epw, Timed{s, h->ev_start, h->ev_stop});
  });
  const int rc = launched("ms_step launch");
  if (rc != MS_OK) return rc;
  // auto-resets that draw a late start (env.py:497-498 -> 406-414), in env order
  if (h->late_on) return launch_late(h, p, done, s);
  return MS_OK;
}

}  // namespace

// csrc/msenv_internal.h: what csrc/mssolve.hip and csrc/msposterior.hip need of a handle
int ms_internal_board_view(ms_handle* h, ms_board_view* out) {
  out->n = h->n;
  out->H = h->H;
  out->W = h->W;
  out->NW = h->NW;
  out->device = h->device;
  out->mine_words = h->mine_words;
  out->rev_words = h->rev_words;
  out->meta = (const uint8_t*)h->meta;
  out->meta_stride = (int32_t)sizeof(EnvMeta);
  out->flags_offset = (int32_t)offsetof(EnvMeta, flags);
  out->avoid_budget = &h->avoid_budget;
  out->mine_count = h->cfg.mine_count;
  out->posterior_budget = &h->posterior_budget;
  return MS_OK;
}

int ms_internal_fail(int code, const char* msg) { return fail(code, "%s", msg); }

extern "C" {

const char* ms_last_error(void) { return g_err; }

int32_t ms_abi_version(void) { return MSENV_ABI_VERSION; }

int ms_create(const ms_cfg* cfg, int64_t n_total, uint64_t base_seed, int64_t env_begin, int64_t env_count,
              ms_handle** out) {
  if (!cfg || !out) return fail(MS_EINVAL, "ms_create: null argument");
  *out = nullptr;
  if (!shape_ok(cfg))
    return fail(MS_EINVAL, "ms_create: unsupported board (need 1<=H<=64, 1<=W<=62, 0<=mine_count<H*W)");
  if (n_total <= 0 || env_begin < 0 || env_count <= 0 || env_begin + env_count > n_total)
    return fail(MS_EINVAL, "ms_create: bad env range");
  if (n_total > (int64_t)1 << 31) return fail(MS_EINVAL, "ms_create: n_total too large");
  ms_handle* h = new (std::nothrow) ms_handle();
  if (!h) return fail(MS_ENOMEM, "ms_create: host allocation failed");
  h->cfg = *cfg;
  h->n_total = n_total;
  h->env_begin = env_begin;
  h->n = env_count;
  h->H = cfg->H;
  h->W = cfg->W;
  h->A = cfg->H * cfg->W;
  const int rpw = 64 / cfg->W;
  h->NW = (cfg->H + rpw - 1) / rpw;
  (void)hipGetDevice(&h->device);
  h->epw = 4;

  // env.py:393-395: base = default_rng(seed); seeds = base.integers(0, 2**31-1, N)
  std::vector<EnvMeta> meta((size_t)env_count);
  HostPcg base;
  host_seed(base, base_seed);
  for (int64_t i = 0; i < env_begin + env_count; ++i) {
    const uint32_t s = host_bounded(base, 2147483646u);
    if (i < env_begin) continue;
    HostPcg r;
    host_seed(r, s);
    EnvMeta& m = meta[(size_t)(i - env_begin)];
    m.st_hi = (uint64_t)(r.state >> 64);
    m.st_lo = (uint64_t)r.state;
    m.inc_hi = (uint64_t)(r.inc >> 64);
    m.inc_lo = (uint64_t)r.inc;
    m.has32 = 0;
    m.uinteger = 0;
    m.step_count = 0;
    m.flags = 0;
  }
  // PCG64 jump-ahead: state after k steps = M^k s + (sum_{i<k} M^i) inc, k = 1..64
  uint64_t jt[64 * 4];
  {
    const unsigned __int128 M = ((unsigned __int128)0x2360ED051FC65DA4ull << 64) | 0x4385DF649FCCF645ull;
    unsigned __int128 Ak = 1, Ck = 0;
    for (int k = 1; k <= 64; ++k) {
      Ck = Ck + Ak;  // sum_{i<k} M^i
      Ak = Ak * M;   // M^k
      jt[4 * (k - 1) + 0] = (uint64_t)(Ak >> 64);
      jt[4 * (k - 1) + 1] = (uint64_t)Ak;
      jt[4 * (k - 1) + 2] = (uint64_t)(Ck >> 64);
      jt[4 * (k - 1) + 3] = (uint64_t)Ck;
    }
  }
  hipError_t e = hipMalloc((void**)&h->meta, sizeof(EnvMeta) * (size_t)env_count);
  if (e == hipSuccess) e = hipMalloc((void**)&h->jump, sizeof(jt));
  if (e == hipSuccess) e = hipMemcpy(h->jump, jt, sizeof(jt), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc((void**)&h->mine_words, sizeof(uint64_t) * (size_t)env_count * h->NW);
  if (e == hipSuccess) e = hipMalloc((void**)&h->rev_words, sizeof(uint64_t) * (size_t)env_count * h->NW);
  if (e == hipSuccess)
    e = hipMemcpy(h->meta, meta.data(), sizeof(EnvMeta) * (size_t)env_count, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(h->mine_words, 0, sizeof(uint64_t) * (size_t)env_count * h->NW);
  if (e == hipSuccess) e = hipMemset(h->rev_words, 0, sizeof(uint64_t) * (size_t)env_count * h->NW);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    const int rc = hip_fail(e, "ms_create");
    ms_destroy(h);
    return rc;
  }
  *out = h;
  return MS_OK;
}

int ms_destroy(ms_handle* h) {
  if (!h) return MS_OK;
  if (h->meta) (void)hipFree(h->meta);
  if (h->mine_words) (void)hipFree(h->mine_words);
  if (h->rev_words) (void)hipFree(h->rev_words);
  if (h->jump) (void)hipFree(h->jump);
  if (h->late_rng) (void)hipFree(h->late_rng);
  delete h;
  return MS_OK;
}

// Diagnostics (not part of msenv.h): per-env s_memtime stamps [env_count][8]
// are written by libmsenv_diag.so (built with -DMS_DIAG); NULL disables.
int ms_set_debug_flags(ms_handle* h, uint32_t flags) {
  if (!h) return fail(MS_EINVAL, "ms_set_debug_flags: null handle");
  h->dbg_flags = flags;
  return MS_OK;
}

int ms_set_timing_events(ms_handle* h, void* start_event, void* stop_event) {
  if (!h) return fail(MS_EINVAL, "ms_set_timing_events: null handle");
  h->ev_start = (hipEvent_t)start_event;
  h->ev_stop = (hipEvent_t)stop_event;
  return MS_OK;
}

int ms_event_create(void** event) {
  if (!event) return fail(MS_EINVAL, "ms_event_create: null argument");
  hipEvent_t e = nullptr;
  hipError_t r = hipEventCreate(&e);
  if (r != hipSuccess) return hip_fail(r, "hipEventCreate");
  *event = (void*)e;
  return MS_OK;
}

int ms_event_elapsed_ms(void* start_event, void* stop_event, float* ms) {
  if (!start_event || !stop_event || !ms) return fail(MS_EINVAL, "ms_event_elapsed_ms: null argument");
  hipError_t r = hipEventElapsedTime(ms, (hipEvent_t)start_event, (hipEvent_t)stop_event);
  return r == hipSuccess ? MS_OK : hip_fail(r, "hipEventElapsedTime");
}

int ms_event_destroy(void* event) {
  if (event) (void)hipEventDestroy((hipEvent_t)event);
  return MS_OK;
}

int ms_set_diag(ms_handle* h, uint64_t* stamps) {
  if (!h) return fail(MS_EINVAL, "ms_set_diag: null handle");
  h->diag = stamps;
  return MS_OK;
}

int ms_reset(ms_handle* h, float* obs, uint8_t* mask, void* stream) {
  if (!h) return fail(MS_EINVAL, "ms_reset: null handle");
  const int64_t work = h->n * 10 * (int64_t)h->A / 4 + 1;
  int blocks = (int)((work + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_reset, dim3(blocks), dim3(256), 0, (hipStream_t)stream, h->meta, h->mine_words,
                     h->rev_words, h->n, h->NW, obs, mask, h->A);
  const int rc = launched("ms_reset launch");
  if (rc != MS_OK) return rc;
  // every env: _reset_env_state (env.py:406-414, 468-477)
  if (h->late_on) return launch_late(h, fill_params(h, obs, mask), nullptr, (hipStream_t)stream);
  return MS_OK;
}

int ms_set_late_start(ms_handle* h, double prob, int32_t min_hidden, int32_t max_hidden, int32_t max_attempts,
                      int32_t max_extra_steps, uint64_t late_seed) {
  if (!h) return fail(MS_EINVAL, "ms_set_late_start: null handle");
  // clamps of env.py:424-430
  LateCfg c;
  c.prob = prob;
  c.min_hidden = min_hidden < 1 ? 1 : min_hidden;
  c.max_hidden = max_hidden < c.min_hidden ? c.min_hidden : max_hidden;
  c.max_attempts = max_attempts < 1 ? 1 : max_attempts;
  c.max_extra_steps = max_extra_steps < 1 ? 1 : max_extra_steps;
  HostPcg r;
  host_seed(r, late_seed);
  Pcg d;
  d.hi = (uint64_t)(r.state >> 64);
  d.lo = (uint64_t)r.state;
  d.ihi = (uint64_t)(r.inc >> 64);
  d.ilo = (uint64_t)r.inc;
  d.has32 = (uint32_t)r.has32;
  d.uinteger = r.uinteger;
  if (!h->late_rng) {
    hipError_t e = hipMalloc(&h->late_rng, sizeof(Pcg));
    if (e != hipSuccess) return hip_fail(e, "ms_set_late_start alloc");
  }
  hipError_t e = hipMemcpy(h->late_rng, &d, sizeof(Pcg), hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(e, "ms_set_late_start copy");
  h->late = c;
  h->late_on = 1;
  h->late_seed = late_seed;
  return MS_OK;
}

int ms_set_late_start_mode(ms_handle* h, int32_t mode) {
  if (!h) return fail(MS_EINVAL, "ms_set_late_start_mode: null handle");
  if (mode != MS_LATE_SHARED && mode != MS_LATE_KEYED) return fail(MS_EINVAL, "ms_set_late_start_mode: bad mode");
  h->late_mode = mode;
  return MS_OK;
}

int ms_late_rng_state(ms_handle* h, uint64_t* out) {
  if (!h || !out) return fail(MS_EINVAL, "ms_late_rng_state: bad argument");
  if (!h->late_rng) return fail(MS_EINVAL, "ms_late_rng_state: late start not configured");
  Pcg d;
  hipError_t e = hipMemcpy(&d, h->late_rng, sizeof(Pcg), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail(e, "ms_late_rng_state copy");
  out[0] = d.hi;
  out[1] = d.lo;
  out[2] = d.ihi;
  out[3] = d.ilo;
  out[4] = d.has32;
  out[5] = d.uinteger;
  return MS_OK;
}

int ms_step(ms_handle* h, const int64_t* actions, float* obs, uint8_t* mask, float* reward, uint8_t* done,
            int32_t* step, int32_t* last_new, double* revealed_frac, int8_t* outcome, void* stream) {
  return do_step(h, actions, 0, obs, mask, reward, done, step, last_new, revealed_frac, outcome, stream);
}

int ms_step_i32(ms_handle* h, const int32_t* actions, float* obs, uint8_t* mask, float* reward, uint8_t* done,
                int32_t* step, int32_t* last_new, double* revealed_frac, int8_t* outcome, void* stream) {
  return do_step(h, actions, 1, obs, mask, reward, done, step, last_new, revealed_frac, outcome, stream);
}

int ms_step_codes(ms_handle* h, const int64_t* actions, uint8_t* codes, uint8_t* mask, float* reward, uint8_t* done,
                  int32_t* step, int32_t* last_new, double* revealed_frac, int8_t* outcome, void* stream) {
  return do_step(h, actions, 0, nullptr, mask, reward, done, step, last_new, revealed_frac, outcome, stream, codes);
}

int ms_run_tape(ms_handle* h, uint64_t t0, int32_t T, int32_t mode, int32_t slots, int64_t* actions, float* obs,
                uint8_t* mask, float* reward, uint8_t* done, int32_t* step, int32_t* last_new, double* revealed_frac,
                int8_t* outcome, void* stream) {
  if (!h) return fail(MS_EINVAL, "ms_run_tape: null handle");
  if (T < 1) return fail(MS_EINVAL, "ms_run_tape: T must be >= 1");
  if (mode != MS_TAPE_UNIFORM && mode != MS_TAPE_SAFE_BIASED) return fail(MS_EINVAL, "ms_run_tape: bad mode");
  if (h->late_on) return fail(MS_EINVAL, "ms_run_tape: late-start resets are not supported");
  const KParams p = fill_params(h, obs, mask, reward, done, step, last_new, revealed_frac, outcome);
  RunParams r;
  r.t0 = t0;
  r.T = T;
  r.mode = mode;
  r.slots = slots ? 1 : 0;
  r.env_begin = h->env_begin;
  r.actions = actions;
  for_shape(StepShapes{}, h->H, h->W, [&](auto sh) {
    using S = decltype(sh);
    launch_run<S::H, S::W>(p, r, Timed{(hipStream_t)stream, h->ev_start, h->ev_stop});
  });
  return launched("ms_run_tape launch");
}

int ms_labels(ms_handle* h, float* mine_labels, uint8_t* mine_valid, void* stream) {
  if (!h) return fail(MS_EINVAL, "ms_labels: null handle");
  hipLaunchKernelGGL(k_labels, dim3((unsigned)h->n), dim3(64), 0, (hipStream_t)stream, h->meta, h->mine_words,
                     h->rev_words, h->n, h->H, h->W, mine_labels, mine_valid);
  return launched("ms_labels launch");
}

int ms_snapshot(ms_handle* h, uint8_t* mine, uint8_t* revealed, uint8_t* counts, uint8_t* first_click,
                int32_t* step_count, void* stream) {
  if (!h) return fail(MS_EINVAL, "ms_snapshot: null handle");
  hipLaunchKernelGGL(k_snapshot, dim3((unsigned)h->n), dim3(64), 0, (hipStream_t)stream, h->meta,
                     h->mine_words, h->rev_words, h->n, h->H, h->W, mine, revealed, counts, first_click,
                     step_count);
  return launched("ms_snapshot launch");
}

int ms_rng_state(ms_handle* h, uint64_t* out, void* stream) {
  if (!h || !out) return fail(MS_EINVAL, "ms_rng_state: null argument");
  hipLaunchKernelGGL(k_rng_state, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     h->meta, h->n, out);
  return launched("ms_rng_state launch");
}

int ms_tape_actions(ms_handle* h, uint64_t t, int32_t mode, int64_t* actions, void* stream) {
  if (!h || !actions) return fail(MS_EINVAL, "ms_tape_actions: null argument");
  if (mode != MS_TAPE_UNIFORM && mode != MS_TAPE_SAFE_BIASED) return fail(MS_EINVAL, "ms_tape_actions: bad mode");
  const uint32_t hw = (uint32_t)h->H | ((uint32_t)h->W << 16);  // H <= 64, W <= 62
  for_shape(TapeShapes{}, h->H, h->W, [&](auto sh) {
    using S = decltype(sh);
    hipLaunchKernelGGL((k_tape<S::H, S::W>), dim3((unsigned)((h->n + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                       h->mine_words, h->rev_words, actions, h->n, h->env_begin, t, (int)mode, hw);
  });
  return launched("ms_tape_actions launch");
}

}  // extern "C"
