// The synthetic tape policy: k_tape (ms_tape_actions) and the same rule evaluated inside the
// multistep kernels, per wave (tape_cell, k_run) and per packed board (pk_tape_cell,
// k_run_packed). Internal to libmsenv.so.
#ifndef MSENV_TAPE_H
#define MSENV_TAPE_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/msenv.h"
#include "msenv_board.h"
#include "msenv_packed.h"
#include "msenv_pcg.h"
#include "msenv_wave.h"

namespace {

// ---------------------------------------------------------------------------
// ms_tape_actions: synthetic policy, one wave per env.
// ---------------------------------------------------------------------------

// One lane per env: the packed row words of a board are its cells in row-major
// order (rows never straddle a word), so "k-th valid cell" is the k-th set bit
// across the NW words of ~revealed (& ~mine). A wave covers 64 boards with
// coalesced 16-B word loads, and the whole launch is a single load round trip
// plus a lane-local tail (k_tape below has the instruction counts).

// The launch is one short dependency chain per lane, so its time is latency: one-wave
// workgroups spread the waves over as many CUs as possible, the board words are loaded once
// (16-B loads) and kept in registers, and the remainder is 32-bit.
//   - Every argument arrives in SGPRs with the wave (kernarg preload): pointers and 64-bit
//     values first, then mode and H | W << 16, 14 dwords in all, so no s_load of the
//     argument segment stands in front of the loads or of the one store.
//   - The hash depends on no loaded word and runs under the load latency: tape_tie makes it
//     an input of the first use of each board word.
//   - The k-th set bit across the NW words is found without branches: a running popcount
//     picks the word (selects), one select_bit64 the bit, and the action is
//     word * (rows per word * W) + bit.
//   - The uniform tape neither loads the mine words nor counts safe cells.
// k_tape<16,16> is 277 instructions, about 230 on the uniform tape's path: ~60 the four 32-bit
// remainders of mod64_small (they share one reciprocal), ~30 the hash, ~45 select_bit64
// (the generic instantiation loops over its words instead).
__device__ __forceinline__ void tape_tie(uint64_t& word, uint64_t x) {
  asm volatile("" : "+v"(word) : "v"(x));
}

template <int H_, int W_>
__global__ __launch_bounds__(64) void k_tape(const uint64_t* mw, const uint64_t* rw, int64_t* actions, int64_t n,
                                             int64_t env_begin, uint64_t t, int mode, uint32_t hw) {
  const int64_t env = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (env >= n) return;
  const Geo<H_, W_> g((int)(hw & 0xffffu), (int)(hw >> 16));
  const int W = g.W, rpw = g.RPW(), NW = g.NW();
  constexpr int kNW = (H_ && W_) ? (H_ + (64 / W_) - 1) / (64 / W_) : 64;
  constexpr bool kStatic = H_ && W_;
  const bool safe_mode = mode == MS_TAPE_SAFE_BIASED;  // (wave-uniform: a kernel argument)
  const uint64_t* rp = rw + env * NW;
  const uint64_t* mp = mw + env * NW;
  auto valid_mask = [&](int w) -> uint64_t {
    const int rows = min(rpw, g.H - w * rpw);
    const int bits = rows * W;
    return bits >= 64 ? ~0ull : ((1ull << bits) - 1ull);
  };
  const uint64_t gidx = (uint64_t)(env_begin + env);
  int64_t act = 0;
  if constexpr (kStatic) {
    // all loads first: the words of a board are contiguous (NW * 8 bytes)
    uint64_t b[kNW], mm[kNW];
#pragma unroll
    for (int w = 0; w < kNW; ++w) b[w] = rp[w];
    if (safe_mode) {
#pragma unroll
      for (int w = 0; w < kNW; ++w) mm[w] = mp[w];
    }
    const uint64_t x = splitmix64(0xC0FFEEull ^ (gidx << 32) ^ t);
#pragma unroll
    for (int w = 0; w < kNW; ++w) tape_tie(b[w], x);
    uint32_t cnt = 0;
#pragma unroll
    for (int w = 0; w < kNW; ++w) {
      b[w] = ~b[w] & valid_mask(w);
      cnt += (uint32_t)__popcll(b[w]);
    }
    uint64_t sel = x;
    if (safe_mode) {
      uint64_t sw[kNW];
      uint32_t n_safe = 0;
#pragma unroll
      for (int w = 0; w < kNW; ++w) {
        sw[w] = b[w] & ~mm[w];
        n_safe += (uint32_t)__popcll(sw[w]);
      }
      sel = x >> 16;
      if ((x & 0xFFFFull) < 65208ull && n_safe > 0) {
        cnt = n_safe;
#pragma unroll
        for (int w = 0; w < kNW; ++w) b[w] = sw[w];
      }
    }
    const uint32_t target = mod64_small(sel, cnt ? cnt : 1u);
    // the word that holds set bit `target`: the last one with fewer than target + 1 set
    // bits in front of it (an empty word never wins: the next one has the same count in front)
    uint64_t bw = b[0];
    uint32_t before = 0, acc = (uint32_t)__popcll(b[0]);
    int base = 0;
#pragma unroll
    for (int w = 1; w < kNW; ++w) {
      const bool here = target >= acc;
      bw = here ? b[w] : bw;
      before = here ? acc : before;
      base = here ? w * rpw * W : base;
      acc += (uint32_t)__popcll(b[w]);
    }
    if (cnt > 0) act = (int64_t)(base + select_bit64(bw, target - before));
  } else {
    uint32_t n_valid = 0, n_safe = 0;
    for (int w = 0; w < NW; ++w) {
      const uint64_t v = ~rp[w] & valid_mask(w);
      n_valid += (uint32_t)__popcll(v);
      if (safe_mode) n_safe += (uint32_t)__popcll(v & ~mp[w]);
    }
    const uint64_t x = splitmix64(0xC0FFEEull ^ (gidx << 32) ^ t);
    const bool want_safe = safe_mode && (x & 0xFFFFull) < 65208ull && n_safe > 0;
    const uint32_t cnt = want_safe ? n_safe : n_valid;
    const uint64_t sel = safe_mode ? (x >> 16) : x;
    if (cnt > 0) {
      uint32_t target = mod64_small(sel, cnt);
      for (int w = 0; w < NW && target != 0xFFFFFFFFu; ++w) {
        uint64_t b = ~rp[w] & valid_mask(w);
        if (want_safe) b &= ~mp[w];
        const uint32_t pc = (uint32_t)__popcll(b);
        if (target < pc) {
          act = (int64_t)(w * rpw * W + select_bit64(b, target));
          target = 0xFFFFFFFFu;  // found
        } else {
          target -= pc;
        }
      }
    }
  }
  actions[env] = act;
}

// The rule of k_tape on a board held one row per lane (k_run): DPP sums, an exclusive scan
// and a k-th-set-bit select.
template <int H_, int W_>
__device__ __forceinline__ int tape_cell(uint64_t mine, uint64_t rev, const Geo<H_, W_>& g, int lane,
                                         uint64_t gidx, uint64_t t, int mode) {
  const uint64_t valid = ~rev & g.rowmask() & (lane < g.H ? ~0ull : 0ull);
  const uint64_t x = splitmix64(0xC0FFEEull ^ (gidx << 32) ^ t);
  uint64_t bits = valid;
  uint32_t cnt = wave_sum((uint32_t)__popcll(valid));
  uint64_t sel = x;
  if (mode == MS_TAPE_SAFE_BIASED) {  // (uniform branch: mode is a kernel argument)
    const uint64_t safe = valid & ~mine;
    const uint32_t n_safe = wave_sum((uint32_t)__popcll(safe));
    sel = x >> 16;
    if ((x & 0xFFFFull) < 65208ull && n_safe > 0) {
      bits = safe;
      cnt = n_safe;
    }
  }
  if (cnt == 0) return 0;
  const uint32_t target = mod64_small(sel, cnt);
  const uint32_t pc = (uint32_t)__popcll(bits);
  const uint32_t before = wave_excl_scan(pc);
  const bool hit = target >= before && target < before + pc;
  const uint64_t who = __ballot(hit);
  const int src = __ffsll((unsigned long long)who) - 1;
  const int col = (int)readlane32((uint32_t)(hit ? select_bit64(bits, target - before) : 0), src);
  return src * g.W + col;
}

// The same on packed boards (k_run_packed): the k-th valid cell is found per board, by board
// sums and a DPP row scan over the board's 16 lanes and the board's bits of one ballot.
template <int H_, int W_, int LPB>
__device__ __forceinline__ int pk_tape_cell(uint32_t mine, uint32_t rev, int lane, uint64_t gidx, uint64_t t, int mode) {
  constexpr uint32_t ROWMASK = (1u << W_) - 1u;
  constexpr uint64_t BM = (1ull << LPB) - 1ull;
  const int r = lane & (LPB - 1);
  const uint32_t valid = ~rev & ROWMASK & (r < H_ ? ~0u : 0u);
  const uint64_t x = splitmix64(0xC0FFEEull ^ (gidx << 32) ^ t);
  uint32_t bits = valid;
  uint32_t cnt = board_sum<LPB>((uint32_t)__popc(valid), lane);
  uint64_t sel = x;
  if (mode == MS_TAPE_SAFE_BIASED) {  // (uniform branch: mode is a kernel argument)
    const uint32_t safe = valid & ~mine;
    const uint32_t n_safe = board_sum<LPB>((uint32_t)__popc(safe), lane);
    sel = x >> 16;
    if ((x & 0xFFFFull) < 65208ull && n_safe > 0) {
      bits = safe;
      cnt = n_safe;
    }
  }
  const uint32_t target = mod64_small(sel, cnt ? cnt : 1u);
  const uint32_t pc = (uint32_t)__popc(bits);
  const uint32_t before = row_excl_scan(pc);
  const bool hit = target >= before && target < before + pc;
  const uint64_t who = (__ballot(hit) >> board_base<LPB>(lane)) & BM;
  const int src = who ? __ffsll((unsigned long long)who) - 1 : 0;
  const int col = (int)board_read<LPB>(hit ? (uint32_t)select_bit64(bits, target - before) : 0u, lane, src);
  return cnt ? src * W_ + col : 0;
}

}  // namespace

#endif  // MSENV_TAPE_H
