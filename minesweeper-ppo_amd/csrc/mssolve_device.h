// Device helpers shared by the one-wavefront-per-board kernels (csrc/mssolve.hip,
// csrc/msposterior.hip): wave shifts and reductions, 3x3 windows over row bitboards (row r at
// index r + 1, column c at bit c + 1) and 128-bit value strings. Internal; every function is
// inlined into its caller.
#ifndef MSSOLVE_DEVICE_H
#define MSSOLVE_DEVICE_H

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace {

__device__ __forceinline__ int lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
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
// one wave per workgroup: a barrier orders the wave's LDS traffic
__device__ __forceinline__ void wave_sync() { __syncthreads(); }
__device__ __forceinline__ uint64_t ballot(bool p) { return __ballot(p); }
__device__ __forceinline__ bool wave_any(bool p) { return __ballot(p) != 0ull; }
__device__ __forceinline__ uint64_t lanes_below(int lane) { return (1ull << lane) - 1ull; }
__device__ __forceinline__ int wave_sum(int v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
  return v;
}

// 3x3 window of plane S around (r, c): bit 3 * (dr + 1) + (dc + 1), the centre is bit 4
__device__ __forceinline__ uint32_t win9(const uint64_t* S, int r, int c) {
  return (uint32_t)((S[r] >> c) & 7ull) | ((uint32_t)((S[r + 1] >> c) & 7ull) << 3) |
         ((uint32_t)((S[r + 2] >> c) & 7ull) << 6);
}
__device__ __forceinline__ void or9(uint64_t* S, int r, int c, uint32_t bits) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint64_t part = (bits >> (3 * k)) & 7u;
    if (part) atomicOr((unsigned long long*)&S[r + k], (unsigned long long)(part << c));
  }
}
__device__ __forceinline__ bool cell_bit(const uint64_t* S, int r, int c) { return (S[r + 1] >> (c + 1)) & 1ull; }
// window bits of the cell at (r, c) moved into the frame of the cell at (r + dr, c + dc);
// lost = some bit falls outside that frame
__device__ __forceinline__ uint32_t shift9(uint32_t m, int dr, int dc, bool& lost) {
  uint32_t out = 0;
  lost = false;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const uint32_t row = (m >> (3 * i)) & 7u;
    const int left = dc < 0 ? -dc : 0, right = dc > 0 ? dc : 0;
    const uint32_t sh = ((row << left) & 7u) >> right;
    const uint32_t back = (sh << right) >> left;
    const int ii = i - dr;
    if (back != row || (row && (ii < 0 || ii > 2))) lost = true;
    if (ii >= 0 && ii <= 2) out |= sh << (3 * ii);
  }
  return out;
}
__device__ __forceinline__ int win_cell(int cell, int W, int k) { return cell + (k / 3 - 1) * W + (k % 3 - 1); }

struct Bits128 {
  uint64_t lo, hi;
};
__device__ __forceinline__ Bits128 bit128(int i) {
  return {i < 64 ? 1ull << i : 0ull, i >= 64 ? 1ull << (i - 64) : 0ull};
}
__device__ __forceinline__ Bits128 below128(int i) {  // bits [0, i), 0 <= i <= 128
  return {i >= 64 ? ~0ull : (1ull << i) - 1ull, i <= 64 ? 0ull : (i >= 128 ? ~0ull : (1ull << (i - 64)) - 1ull)};
}

}  // namespace

#endif  // MSSOLVE_DEVICE_H
