// mssym.hip — the board symmetries on the device (C ABI include/mssym.h).
//
// All three kernels have k_expert's shape: one wavefront per row, four rows per workgroup, lane l
// owns the OUTPUT cells l, l + 64, ... (at most 8), so stores are coalesced; the source cell of
// each comes from mssym::source_cell (mssym_map.h). No LDS, no atomics, no scratch; every output
// element is written by exactly one lane, with plain vector stores.
//
//   k_sym_gather  output row i = T_{g[i]} of source row rows[i], five planes in one launch
//   k_sym_expand  source row i -> its G images, out[g, i] = T_g(codes[i])
//   k_sym_mean    out[i, c] = (1/G) * pairwise tree over g of x[g, i, cell of c in image g]
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/mssym.h"
#include "msenv_internal.h"
#include "mssym_map.h"

namespace {

constexpr int kWave = 64;
constexpr int kRowsPerBlock = 4;
constexpr int kMaxQ = MS_AVOID_MAX_CELLS / kWave;  // 64-cell slices of the largest board
static_assert(kMaxQ * kWave == MS_AVOID_MAX_CELLS, "whole slices");

struct SymPlanes {
  const uint8_t* codes;
  const uint8_t* mask;
  const uint8_t* best;
  const uint32_t* labels;  // f32 moved as bits
  const uint8_t* kind;
  uint8_t* codes_out;
  uint8_t* mask_out;
  uint8_t* best_out;
  uint32_t* labels_out;
  uint8_t* kind_out;
  uint8_t* status;
};

__global__ __launch_bounds__(kWave* kRowsPerBlock) void k_sym_gather(const int64_t* __restrict__ rows,
                                                                      const uint8_t* __restrict__ g, int64_t n, int H,
                                                                      int W, int64_t B_src, SymPlanes p) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t i = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (i >= n) return;
  const int A = H * W;
  const int64_t src = rows ? rows[i] : i;
  const unsigned gi = g[i];
  // a bad row reads nothing and is written as zeros: nothing is clamped
  const bool ok = src >= 0 && src < B_src && mssym::valid(H, W, gi);
  const int64_t so = ok ? src * A : 0, oo = i * A;
#pragma unroll
  for (int q = 0; q < kMaxQ; ++q) {
    const int c = lane + kWave * q;
    if (c >= A) break;
    const int s = ok ? mssym::source_cell(H, W, gi, c) : 0;
    if (p.codes && p.codes_out) p.codes_out[oo + c] = ok ? p.codes[so + s] : (uint8_t)0;
    if (p.mask && p.mask_out) p.mask_out[oo + c] = ok ? p.mask[so + s] : (uint8_t)0;
    if (p.best && p.best_out) p.best_out[oo + c] = ok ? p.best[so + s] : (uint8_t)0;
    if (p.labels && p.labels_out) p.labels_out[oo + c] = ok ? p.labels[so + s] : 0u;
  }
  if (lane == 0) {
    if (p.kind && p.kind_out) p.kind_out[i] = ok ? p.kind[src] : (uint8_t)0;
    if (p.status) p.status[i] = ok ? 0 : 1;
  }
}

__global__ __launch_bounds__(kWave* kRowsPerBlock) void k_sym_expand(const uint8_t* __restrict__ codes, int64_t n,
                                                                      int H, int W, int G, uint8_t* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t i = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (i >= n) return;
  const int A = H * W;
  const uint8_t* in = codes + i * A;
  for (int g = 0; g < G; ++g) {
    uint8_t* o = out + ((int64_t)g * n + i) * A;
#pragma unroll
    for (int q = 0; q < kMaxQ; ++q) {
      const int c = lane + kWave * q;
      if (c >= A) break;
      o[c] = in[mssym::source_cell(H, W, (unsigned)g, c)];
    }
  }
}

// the cell of image g that belongs to the original cell c: T_g maps it to c's place, so it is
// where T_{inverse(g)} reads from
__device__ inline float image_value(const float* __restrict__ x, int64_t n, int64_t i, int H, int W, int g, int c) {
  return x[((int64_t)g * n + i) * (H * W) + mssym::source_cell(H, W, mssym::inverse((unsigned)g), c)];
}

template <int G>
__global__ __launch_bounds__(kWave* kRowsPerBlock) void k_sym_mean(const float* __restrict__ x, int64_t n, int H,
                                                                    int W, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t i = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (i >= n) return;
  const int A = H * W;
#pragma unroll
  for (int q = 0; q < kMaxQ; ++q) {
    const int c = lane + kWave * q;
    if (c >= A) break;
    float y[G];
#pragma unroll
    for (int g = 0; g < G; ++g) y[g] = image_value(x, n, i, H, W, g, c);
    float s = y[0];
    if constexpr (G == 4) s = (y[0] + y[1]) + (y[2] + y[3]);
    if constexpr (G == 8) s = ((y[0] + y[1]) + (y[2] + y[3])) + ((y[4] + y[5]) + (y[6] + y[7]));
    out[i * A + c] = s * (1.0f / G);
  }
}

int fail(const char* who, const char* what) {
  char msg[160];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return ms_internal_fail(MS_EINVAL, msg);
}

int shape_bad(const char* who, int32_t H, int32_t W) {
  if (H < 1 || W < 1 || H > MS_AVOID_MAX_CELLS || W > MS_AVOID_MAX_CELLS || H * W > MS_AVOID_MAX_CELLS)
    return fail(who, "need 1 <= H, W and H*W <= 512");
  return MS_OK;
}

int rows_bad(const char* who, int64_t n) {
  if (n <= 0 || n > 0x7fffffffll) return fail(who, "need 1 <= n < 2^31");
  return MS_OK;
}

int group_bad(const char* who, int32_t H, int32_t W, int32_t G) {
  if (G != 1 && G != 4 && G != 8) return fail(who, "G must be 1, 4 or 8");
  if (G == 8 && H != W) return fail(who, "G = 8 needs a square board");
  return MS_OK;
}

int launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return MS_OK;
  char msg[256];
  snprintf(msg, sizeof msg, "%s launch: %s", who, hipGetErrorString(e));
  return ms_internal_fail(MS_EHIP, msg);
}

unsigned grid_of(int64_t n) { return (unsigned)((n + kRowsPerBlock - 1) / kRowsPerBlock); }

}  // namespace

extern "C" {

int ms_sym_cell_map_host(int32_t H, int32_t W, int32_t g, int32_t* map) {
  const char* who = "ms_sym_cell_map_host";
  if (int rc = shape_bad(who, H, W)) return rc;
  if (!map) return fail(who, "null map");
  if (g < 0 || !mssym::valid(H, W, (unsigned)g)) return fail(who, "g must be 0..3, or 0..7 on a square board");
  if (mssym::cell_map_host(H, W, g, map, MS_AVOID_MAX_CELLS)) return fail(who, "bad argument");
  return MS_OK;
}

int ms_sym_gather(const int64_t* rows, const uint8_t* g, int64_t n, int32_t H, int32_t W, int64_t B_src,
                  const uint8_t* codes, const uint8_t* mask, const uint8_t* best, const float* labels,
                  const uint8_t* kind, uint8_t* codes_out, uint8_t* mask_out, uint8_t* best_out, float* labels_out,
                  uint8_t* kind_out, uint8_t* status, void* stream) {
  const char* who = "ms_sym_gather";
  if (int rc = shape_bad(who, H, W)) return rc;
  if (int rc = rows_bad(who, n)) return rc;
  if (!g) return fail(who, "null g");
  if (B_src < 1 || B_src > 0x7fffffffll) return fail(who, "need 1 <= B_src < 2^31");
  if (!rows && n != B_src) return fail(who, "null rows is the identity: it needs n == B_src");
  const SymPlanes p = {codes,     mask,     best,     (const uint32_t*)labels, kind,  codes_out,
                       mask_out,  best_out, (uint32_t*)labels_out,             kind_out, status};
  hipLaunchKernelGGL(k_sym_gather, dim3(grid_of(n)), dim3(kWave * kRowsPerBlock), 0, (hipStream_t)stream, rows, g, n,
                     (int)H, (int)W, B_src, p);
  return launched(who);
}

int ms_sym_expand(const uint8_t* codes, int64_t n, int32_t H, int32_t W, int32_t G, uint8_t* out, void* stream) {
  const char* who = "ms_sym_expand";
  if (int rc = shape_bad(who, H, W)) return rc;
  if (int rc = rows_bad(who, n)) return rc;
  if (int rc = group_bad(who, H, W, G)) return rc;
  if (!codes || !out) return fail(who, "null codes or out");
  hipLaunchKernelGGL(k_sym_expand, dim3(grid_of(n)), dim3(kWave * kRowsPerBlock), 0, (hipStream_t)stream, codes, n,
                     (int)H, (int)W, (int)G, out);
  return launched(who);
}

int ms_sym_mean(const float* x, int64_t n, int32_t H, int32_t W, int32_t G, float* out, void* stream) {
  const char* who = "ms_sym_mean";
  if (int rc = shape_bad(who, H, W)) return rc;
  if (int rc = rows_bad(who, n)) return rc;
  if (int rc = group_bad(who, H, W, G)) return rc;
  if (!x || !out) return fail(who, "null x or out");
  const dim3 grid(grid_of(n)), block(kWave * kRowsPerBlock);
  const hipStream_t s = (hipStream_t)stream;
  if (G == 8)
    hipLaunchKernelGGL(k_sym_mean<8>, grid, block, 0, s, x, n, (int)H, (int)W, out);
  else if (G == 4)
    hipLaunchKernelGGL(k_sym_mean<4>, grid, block, 0, s, x, n, (int)H, (int)W, out);
  else
    hipLaunchKernelGGL(k_sym_mean<1>, grid, block, 0, s, x, n, (int)H, (int)W, out);
  return launched(who);
}

}  // extern "C"
