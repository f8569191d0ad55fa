// A board as the env kernels hold it (csrc/msenv.hip): the per-env record in HBM, the kernel
// parameter block, the packed row words and their geometry, and everything a step writes
// out -- the observation planes with their store forms, the mask and codes, the aux outputs
// and the state write-back. Internal to libmsenv.so.
#ifndef MSENV_BOARD_H
#define MSENV_BOARD_H

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "msenv_pcg.h"
#include "msenv_wave.h"

namespace {

constexpr int kMaxH = 64;
constexpr int kMaxW = 62;

// ---------------------------------------------------------------------------
// Per-env persistent state in HBM (array of structs, 48 B per env).
// ---------------------------------------------------------------------------
struct alignas(16) EnvMeta {
  uint64_t st_hi, st_lo, inc_hi, inc_lo;  // PCG64 state / increment
  uint32_t has32, uinteger;               // numpy next_uint32 half-word buffer
  int32_t step_count;
  uint32_t flags;                         // bit0: first_click_done
};
static_assert(sizeof(EnvMeta) == 48, "EnvMeta layout");

struct KParams {
  const void* actions;   // int64 or int32 [n]
  float* obs;            // [n,10,H,W]
  uint8_t* mask;         // [n,A]
  float* reward;
  uint8_t* done;
  int32_t* step;
  int32_t* last_new;
  double* frac;
  int8_t* outcome;
  EnvMeta* meta;
  uint64_t* mine_words;  // [n, NW] packed rows
  uint64_t* rev_words;   // [n, NW]
  int64_t n;
  int32_t H, W, K, guarantee;
  int32_t actions_i32;
  double win_reward, loss_reward, step_penalty;
  const uint64_t* jump;  // [64][4] PCG64 jump-ahead table {A_hi, A_lo, C_hi, C_lo}, k = 1..64
  uint64_t* diag;        // MS_DIAG builds only: per-env s_memtime stamps [n][8]
  uint32_t dbg_flags;    // MS_DBG_* (msenv_debug.h)
  uint8_t* codes;        // [n,A] cell codes (ms_step_codes: 0 hidden, 1 + k revealed with k), or NULL
};

// k_step reads the KParams fields behind its preloaded words (the output pointers, the
// rewards, K / guarantee, dbg_flags, codes) where it first uses them, after the click. Each
// launch has its own argument block, so the first scalar load from each 64-byte line of it
// misses to memory, on the wave's serial path. kparams_warm issues one dword load per line at
// the top of the kernel and kparams_warm_wait retires them behind the prologue's vector-load
// wait, where the wave stands still anyway. The compiler merges most touches with the fields'
// own loads, which then issue beside the vector loads and hold their SGPRs from there on (it
// spills some to VGPR lanes; accepted); a field it still loads late hits the scalar cache.
// The touched fields are less than 64 bytes apart from obs to codes, so every line in that
// range is touched whatever the block's alignment.
struct KParamsWarm {
  uint32_t w[5];
};
__device__ __forceinline__ uint32_t kparams_dword(const void* field) {
  return *reinterpret_cast<const uint32_t*>(field);
}
__device__ __forceinline__ KParamsWarm kparams_warm(const KParams& p) {
  static_assert(offsetof(KParams, outcome) - offsetof(KParams, obs) < 64 &&
                    offsetof(KParams, guarantee) - offsetof(KParams, outcome) < 64 &&
                    offsetof(KParams, step_penalty) - offsetof(KParams, guarantee) < 64 &&
                    offsetof(KParams, codes) - offsetof(KParams, step_penalty) < 64 &&
                    sizeof(KParams) - offsetof(KParams, codes) <= 8,
                "kparams_warm: one touch per 64-byte line");
  KParamsWarm k;
  k.w[0] = kparams_dword(&p.obs);
  k.w[1] = kparams_dword(&p.outcome);
  k.w[2] = kparams_dword(&p.guarantee);
  k.w[3] = kparams_dword(&p.step_penalty);
  k.w[4] = kparams_dword(&p.codes);
  return k;
}
__device__ __forceinline__ void kparams_warm_wait(const KParamsWarm& k) {
  asm volatile("" ::"s"(k.w[0]), "s"(k.w[1]), "s"(k.w[2]), "s"(k.w[3]), "s"(k.w[4]));
}

// ---------------------------------------------------------------------------
// Obs plane stores. The f32 observation is ~97 % of the bytes a step writes and nothing in
// the launch reads it back, so every kernel that writes it (k_step, k_step_packed, k_run,
// k_run_packed, k_reset) goes through these two helpers, and MS_OBS_STORE picks the store
// form at compile time (one library per form for an A/B, no branch in the kernel):
//   0  plain: the lines stay dirty in the XCD's L2 until evicted or the kernel-end release
//   1  non-temporal (global_store_dwordx4 ... nt): the line stays in L2, marked streaming
//   2  write-through (global_store_dwordx4 ... sc1): the line leaves L2 with the store, so
//      the kernel-end release finds it clean; only the 16-B form (a 4-B write-through
//      store costs ~6x the 16-B one per byte, so the scalar form, which only odd-sized
//      boards and partial tails take, stays plain)
// State (store_meta, store_rows), aux, the u8 codes and the mask are read by the next
// kernels and stay plain stores. Write-through is the default: at 16x16x40 with 4,096 envs
// it measured +15 % env-steps/s over plain and nt +11.5 % (DESIGN.md §3, round 7;
// profiles/r07/store_policy_micro.txt, obs_store_ab.txt).
// ---------------------------------------------------------------------------
#ifndef MS_OBS_STORE
#define MS_OBS_STORE 2
#endif
static_assert(MS_OBS_STORE >= 0 && MS_OBS_STORE <= 2, "MS_OBS_STORE: 0 plain, 1 nt, 2 write-through");
constexpr int kObsStore = MS_OBS_STORE;
// The lane-packed small-board kernels (pk_emit: four 9x9 / 8x8 boards per wave as one
// contiguous span whose ends share 128-B lines with the neighbouring waves') lose with
// write-through, 9x9x10 @ 8,192: step 655 M env-steps/s plain, 758 nt, 600 write-through;
// multistep 1.35 G plain, 1.28 nt, 1.06 write-through (profiles/r07/pk_emit_9x9.txt). So where
// the library's form is write-through, k_step_packed's pk_emit stores nt and k_run_packed's plain.
constexpr int kObsStorePackedStep = kObsStore == 2 ? 1 : kObsStore;
constexpr int kObsStorePackedRun = kObsStore == 2 ? 0 : kObsStore;
typedef float f32x4_t __attribute__((ext_vector_type(4)));

template <int FORM = kObsStore>
__device__ __forceinline__ void store_plane4(float4* p, float4 v) {
  if constexpr (FORM == 1) {
    f32x4_t x = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(x, reinterpret_cast<f32x4_t*>(p));
  } else if constexpr (FORM == 2) {
    f32x4_t x = {v.x, v.y, v.z, v.w};
    // s_nop 1: the two wait states before the compiler's next instruction may overwrite the
    // store's data registers (it tracks that hazard only for its own stores). The store counts
    // on vmcnt like any other; a later wait of the compiler's can only wait longer for it.
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1"
                 :
                 : "v"((__attribute__((address_space(1))) f32x4_t*)p), "v"(x)
                 : "memory");
  } else {
    *p = v;
  }
}
template <int FORM = kObsStore>
__device__ __forceinline__ void store_plane1(float* p, float v) {
  if constexpr (FORM == 1) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// ---------------------------------------------------------------------------
// Board geometry: compile-time for the benchmark shapes, runtime otherwise.
// Rows are packed RPW = floor(64/W) rows per u64 word (no row straddles a
// word): 16x16 -> 4 words (32 B/plane), 9x9 -> 2, 30x16 -> 8, 16x30 -> 8.
// ---------------------------------------------------------------------------
template <int H_, int W_>
struct Geo {
  int H, W;
  __device__ __forceinline__ Geo(int h, int w) : H(H_ ? H_ : h), W(W_ ? W_ : w) {}
  __device__ __forceinline__ int A() const { return H * W; }
  __device__ __forceinline__ int RPW() const { return 64 / W; }
  __device__ __forceinline__ int NW() const { return (H + RPW() - 1) / RPW(); }
  __device__ __forceinline__ uint64_t rowmask() const { return (1ull << W) - 1ull; }
};

template <int H_, int W_>
__device__ __forceinline__ uint64_t load_row(const uint64_t* words, const Geo<H_, W_>& g, int lane) {
  // no branch around the load: lanes past the board read a valid word (clamped index)
  // and are masked afterwards, so the compiler can issue every load of the kernel's
  // prologue back to back instead of waiting out each one inside a divergent branch
  const int rpw = g.RPW();
  const int w = lane / rpw;
  const int wc = w < g.NW() ? w : g.NW() - 1;
  const int sh = (lane - w * rpw) * g.W;
  const uint64_t v = words[wc];
  const uint64_t keep = 0ull - (uint64_t)(lane < g.H);  // a mask, not a select: a select
  return (v >> sh) & g.rowmask() & keep;                 // lets the load sink into a branch
}

// rows -> packed words. rows-per-word a power of two (W=16: 4, W=30: 2, W=8: 8,
// W>32: 1): OR the lane group's shifted rows with DPP (quad_perm xor1/xor2,
// row_half_mirror, row_mirror), no LDS. Otherwise (W=9: 7 rows/word) through
// LDS (srow: this wave's 64-entry row buffer).
template <int H_, int W_>
__device__ __forceinline__ void store_rows(uint64_t* words, uint64_t row, uint64_t* srow,
                                           const Geo<H_, W_>& g, int lane) {
  const int nw = g.NW(), rpw = g.RPW();
  if ((rpw & (rpw - 1)) == 0 && rpw <= 16) {
    uint64_t v = row << ((lane & (rpw - 1)) * g.W);
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    if (rpw >= 2) { lo |= dpp32<0xB1>(lo); hi |= dpp32<0xB1>(hi); }
    if (rpw >= 4) { lo |= dpp32<0x4E>(lo); hi |= dpp32<0x4E>(hi); }
    if (rpw >= 8) { lo |= dpp32<0x141>(lo); hi |= dpp32<0x141>(hi); }
    if (rpw >= 16) { lo |= dpp32<0x140>(lo); hi |= dpp32<0x140>(hi); }
    const int w = lane / rpw;
    if ((lane & (rpw - 1)) == 0 && w < nw) words[w] = ((uint64_t)hi << 32) | lo;
    return;
  }
  srow[lane] = row;
  wave_sync();
  if (lane < nw) {
    uint64_t acc = 0;
    for (int k = 0; k < rpw; ++k) {
      const int r = lane * rpw + k;
      if (r < g.H) acc |= srow[r] << (k * g.W);
    }
    words[lane] = acc;
  }
  wave_sync();
}

// ---------------------------------------------------------------------------
// Per-cell observation code: 0 hidden, 1+count revealed, 10 revealed with no
// count plane (first_click_done False; unreachable but exact).
// sM: padded mine rows shifted left by one (sM[r+1] = mine_r << 1).
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t cell_code(const uint64_t* sR, const uint64_t* sM, int r, int c, bool fc) {
  const uint32_t rv = (uint32_t)(sR[r] >> c) & 1u;
  const uint64_t up = sM[r] >> c, mid = sM[r + 1] >> c, dn = sM[r + 2] >> c;
  const uint32_t cnt = (uint32_t)__popcll(up & 7ull) + (uint32_t)__popcll(dn & 7ull) +
                       (uint32_t)(mid & 1ull) + (uint32_t)((mid >> 2) & 1ull);
  return rv ? (fc ? 1u + cnt : 10u) : 0u;
}

// Writes obs [10,A] f32 and mask [A] u8 of one env from the LDS rows. (sCode: A bytes of
// this wave's LDS scratch, reserved for a code-staged emit; a flat 8-B stream of the
// env's 10*A floats measured slower on 9x9 than the per-cell stores below.)
// codes (may be NULL): the cell codes of the obs (1 + count where plane 1 + count is set; the
// unreachable code 10 -- revealed before the first click, plane 0 only -- becomes 0, as
// mc_obs_encode reads such an obs), 4-B aligned when A % 4 == 0.
template <int H_, int W_>
__device__ __forceinline__ void emit_obs(float* __restrict__ obs, uint8_t* __restrict__ mask,
                                         uint8_t* __restrict__ codes, const uint64_t* sR, const uint64_t* sM,
                                         bool fc, const Geo<H_, W_>& g, int lane, uint8_t* sCode) {
  const int A = g.A(), W = g.W;
  if ((A & 3) == 0) {
    const int nq = A >> 2;
    for (int q = lane; q < nq; q += kWave) {
      uint32_t code[4];
      if ((W & 3) == 0) {  // the quad lies in one row: 4 LDS reads for 4 cells
        const int r = (4 * q) / W, c0 = 4 * q - r * W;
        const uint32_t rv = (uint32_t)(sR[r] >> c0);
        const uint64_t up = sM[r] >> c0, mid = sM[r + 1] >> c0, dn = sM[r + 2] >> c0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t cnt = (uint32_t)__popcll((up >> k) & 7ull) + (uint32_t)__popcll((dn >> k) & 7ull) +
                               (uint32_t)((mid >> k) & 1ull) + (uint32_t)((mid >> (k + 2)) & 1ull);
          code[k] = ((rv >> k) & 1u) ? (fc ? 1u + cnt : 10u) : 0u;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int i = 4 * q + k;
          const int r = i / W, c = i - (i / W) * W;
          code[k] = cell_code(sR, sM, r, c, fc);
        }
      }
      if (obs) {
        float4* o4 = reinterpret_cast<float4*>(obs) + q;
        const int stride4 = A >> 2;
        float4 v;
        v.x = code[0] ? 1.f : 0.f;
        v.y = code[1] ? 1.f : 0.f;
        v.z = code[2] ? 1.f : 0.f;
        v.w = code[3] ? 1.f : 0.f;
        store_plane4(o4, v);
#pragma unroll
        for (uint32_t ch = 1; ch < 10; ++ch) {
          v.x = code[0] == ch ? 1.f : 0.f;
          v.y = code[1] == ch ? 1.f : 0.f;
          v.z = code[2] == ch ? 1.f : 0.f;
          v.w = code[3] == ch ? 1.f : 0.f;
          store_plane4(o4 + ch * stride4, v);
        }
      }
      if (mask) {
        const uint32_t m = (code[0] ? 0u : 1u) | ((code[1] ? 0u : 1u) << 8) |
                           ((code[2] ? 0u : 1u) << 16) | ((code[3] ? 0u : 1u) << 24);
        reinterpret_cast<uint32_t*>(mask)[q] = m;
      }
      if (codes) {
        uint32_t cw = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) cw |= (code[k] == 10u ? 0u : code[k]) << (8 * k);
        reinterpret_cast<uint32_t*>(codes)[q] = cw;
      }
    }
  } else {
    (void)sCode;
    for (int i = lane; i < A; i += kWave) {
      const int r = i / W, c = i - (i / W) * W;
      const uint32_t code = cell_code(sR, sM, r, c, fc);
      if (obs) {
        store_plane1(obs + i, code ? 1.f : 0.f);
#pragma unroll
        for (uint32_t ch = 1; ch < 10; ++ch) store_plane1(obs + ch * A + i, code == ch ? 1.f : 0.f);
      }
      if (mask) mask[i] = code ? 0 : 1;
      if (codes) codes[i] = (uint8_t)(code == 10u ? 0u : code);
    }
  }
}

template <int H_, int W_>
__device__ __forceinline__ void stage_rows(uint64_t* sR, uint64_t* sM, uint64_t rev, uint64_t mine,
                                           const Geo<H_, W_>& g, int lane) {
  sR[lane] = rev;
  sM[lane + 1] = mine << 1;
  if (lane == 0) {
    sM[0] = 0ull;
    sM[kWave + 1] = 0ull;
  }
  wave_sync();
}

// Step outputs of one env in three store instructions, one per element width: lanes
// 0..2 write the 4-byte fields (reward, step, last_new), lanes 0..1 the 1-byte fields
// (done, outcome), lane 0 revealed_frac. Reported before the auto-reset (env.py:492-505).
__device__ __forceinline__ void store_aux(const KParams& p, int64_t idx, int lane, double reward, bool done,
                                          int32_t step_count, uint32_t newly, uint32_t total_rev, int outcome, int A) {
  // The pointers become scalar values before the per-lane select: selecting between the
  // fields themselves compiles to a lane-indexed load from the kernel arguments, and its
  // vmcnt(0) waits for every store in flight (in k_run: the previous step's obs). Global
  // address space: a generic pointer would become a flat store, which also counts in
  // lgkmcnt and so holds up the LDS waits behind it.
  typedef __attribute__((address_space(1))) uint32_t gu32;
  typedef __attribute__((address_space(1))) uint8_t gu8;
  const uint64_t pr = rfl64((uint64_t)p.reward), ps = rfl64((uint64_t)p.step), pl = rfl64((uint64_t)p.last_new);
  const uint64_t pd = rfl64((uint64_t)p.done), po = rfl64((uint64_t)p.outcome);
  gu32* d4 = (gu32*)(lane == 0 ? pr : (lane == 1 ? ps : pl));
  const uint32_t v4 = lane == 0 ? __float_as_uint((float)reward) : (lane == 1 ? (uint32_t)step_count : newly);
  if (lane < 3 && d4) d4[idx] = v4;
  gu8* d1 = (gu8*)(lane == 0 ? pd : po);
  const uint8_t v1 = lane == 0 ? (uint8_t)(done ? 1 : 0) : (uint8_t)(int8_t)outcome;
  if (lane < 2 && d1) d1[idx] = v1;
  if (lane == 0 && p.frac) p.frac[idx] = (double)total_rev / (double)(A > 1 ? A : 1);
}

// EnvMeta write-back in two 16-B stores: {st_hi, st_lo} and {has32, uinteger, step_count, flags}
__device__ __forceinline__ void store_meta(EnvMeta* mp, const Pcg& rng, int32_t step_count, bool fc, int lane) {
  if (lane == 0) {
    *reinterpret_cast<ulonglong2*>(&mp->st_hi) = make_ulonglong2(rng.hi, rng.lo);
    *reinterpret_cast<uint4*>(&mp->has32) =
        make_uint4(rng.has32, rng.uinteger, (uint32_t)step_count, fc ? 1u : 0u);
  }
}

}  // namespace

#endif  // MSENV_BOARD_H
