// Wave-level primitives of the env kernels (csrc/msenv.hip, csrc/msrollout.hip): lane id,
// readfirstlane / readlane, DPP moves, the wave-local LDS barrier, sums and scans, k-th set
// bit, a 32-bit remainder. Internal to libmsenv.so; everything here is inlined.
#ifndef MSENV_WAVE_H
#define MSENV_WAVE_H

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace {

constexpr int kWave = 64;

// ---------------------------------------------------------------------------
// Wave helpers
// ---------------------------------------------------------------------------
__device__ __forceinline__ int lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

__device__ __forceinline__ uint32_t rfl(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint64_t rfl64(uint64_t x) {
  return ((uint64_t)rfl((uint32_t)(x >> 32)) << 32) | rfl((uint32_t)x);
}

// DPP moves (gfx9 family): wave_shr:1 = lane r <- lane r-1, wave_shl:1 =
// lane r <- lane r+1, row_shr:n = lane r <- lane r-n inside a 16-lane row;
// bound_ctrl fills out-of-range sources with 0. One VALU op each, no LDS.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
__device__ __forceinline__ uint64_t wave_shr1(uint64_t v) {  // lane r <- lane r-1 (lane 0 <- 0)
  return ((uint64_t)dpp32<0x138>((uint32_t)(v >> 32)) << 32) | dpp32<0x138>((uint32_t)v);
}
__device__ __forceinline__ uint64_t wave_shl1(uint64_t v) {  // lane r <- lane r+1 (lane 63 <- 0)
  return ((uint64_t)dpp32<0x130>((uint32_t)(v >> 32)) << 32) | dpp32<0x130>((uint32_t)v);
}
__device__ __forceinline__ uint32_t row_shr1(uint32_t v) { return dpp32<0x111>(v); }  // r <- r-1; r=0 <- 0
__device__ __forceinline__ uint32_t row_shl1(uint32_t v) { return dpp32<0x101>(v); }  // r <- r+1; r=15 <- 0
__device__ __forceinline__ uint32_t readlane32(uint32_t v, int l) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
  return ((uint64_t)readlane32((uint32_t)(v >> 32), l) << 32) | readlane32((uint32_t)v, l);
}
__device__ __forceinline__ uint32_t bperm(uint32_t v, int src_lane) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)v);
}
// Wave-local LDS barrier. A workgroup of k_step / k_tape holds several boards,
// one per wave, each with its own LDS region, so a board's LDS exchanges only
// have to be ordered inside its wave: a wave's DS operations execute in issue
// order, so this is a compiler code-motion fence plus a wait for outstanding
// LDS results, not an s_barrier (waves of one workgroup never wait for each other).
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// wave-wide sum: 4 DPP row-prefix adds + 4 readlanes (uniform result)
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  v += dpp32<0x111>(v);
  v += dpp32<0x112>(v);
  v += dpp32<0x114>(v);
  v += dpp32<0x118>(v);
  return readlane32(v, 15) + readlane32(v, 31) + readlane32(v, 47) + readlane32(v, 63);
}

// exclusive prefix sum inside each 16-lane row (row_shr 1/2/4/8)
__device__ __forceinline__ uint32_t row_excl_scan16(uint32_t v) {
  uint32_t s = v;
  s += dpp32<0x111>(s);
  s += dpp32<0x112>(s);
  s += dpp32<0x114>(s);
  s += dpp32<0x118>(s);
  return s - v;
}

__device__ __forceinline__ uint32_t row_excl_scan(uint32_t v) {  // inside one 16-lane DPP row
  uint32_t s = v;
  s += dpp32<0x111>(s);
  s += dpp32<0x112>(s);
  s += dpp32<0x114>(s);
  s += dpp32<0x118>(s);
  return s - v;
}

// exclusive prefix sum over the wave: Kogge-Stone inside 16-lane rows
// (row_shr 1/2/4/8), then row_bcast15 / row_bcast31 carry across rows (GFX9 DPP)
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v) {
  uint32_t s = v;
  s += dpp32<0x111>(s);
  s += dpp32<0x112>(s);
  s += dpp32<0x114>(s);
  s += dpp32<0x118>(s);
  s += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x142, 0xa, 0xf, false);
  s += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x143, 0xc, 0xf, false);
  return s - v;
}

__device__ __forceinline__ int select_bit64(uint64_t x, uint32_t k) {  // k-th set bit, k < popc(x)
  int pos = 0;
#pragma unroll
  for (int half = 32; half >= 1; half >>= 1) {
    const uint64_t lowmask = (1ull << half) - 1ull;
    const uint32_t c = (uint32_t)__popcll(x & lowmask);
    if (k >= c) {
      k -= c;
      x >>= half;
      pos += half;
    }
  }
  return pos;
}

__device__ __forceinline__ int select_bit32(uint32_t x, uint32_t k) {  // k-th set bit, k < popc(x)
  int pos = 0;
#pragma unroll
  for (int half = 16; half >= 1; half >>= 1) {
    const uint32_t c = (uint32_t)__popc(x & ((1u << half) - 1u));
    if (k >= c) {
      k -= c;
      x >>= half;
      pos += half;
    }
  }
  return pos;
}

// x mod c for c <= 65535 in 32-bit arithmetic (a 64-bit remainder is a long
// software sequence on the GPU): x = hi * 2^32 + lo, 2^32 mod c = (2^32 - c) mod c
__device__ __forceinline__ uint32_t mod64_small(uint64_t x, uint32_t c) {
  const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
  const uint32_t r = ((hi % c) * ((0u - c) % c)) % c;  // < c^2 < 2^32
  const uint32_t s = r + lo % c;                        // < 2c
  return s >= c ? s - c : s;
}

}  // namespace

#endif  // MSENV_WAVE_H
