// msrollout.hip — the rollout kernels of include/msenv.h that never touch a board: GAE, the
// masked Gumbel-max sampler and the Dropout2d channel masks. Reference behaviour followed
// (yakvrz/minesweeper-ppo):
//   RolloutBuffer.compute_gae      minesweeper/buffers.py:78-94
//   masked Categorical sampling    train_rl.py:229-235
// Built with the flags of msenv.hip (Makefile); errors go through ms_internal_fail into the
// buffer that ms_last_error reads.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "../../include/msenv.h"
#include "msenv_internal.h"
#include "msenv_pcg.h"
#include "msenv_wave.h"

namespace {

// ---------------------------------------------------------------------------
// ms_gae: thread per env, reverse scan over T, reference f32 op order
// (buffers.py:87-94) with explicit round-to-nearest ops (no contraction).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gae(const float* __restrict__ rewards, const float* __restrict__ values,
                                             const uint8_t* __restrict__ dones, const float* __restrict__ last_values,
                                             int T, int64_t N, float gamma, float gl, float* __restrict__ adv,
                                             float* __restrict__ ret) {
#pragma clang fp contract(off)
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float last_adv = 0.f;
  float nv = last_values[n];
  for (int t = T - 1; t >= 0; --t) {
    const int64_t i = (int64_t)t * N + n;
    const float v = values[i];
    // plain operators under `fp contract(off)`: each op rounds to f32 (the
    // __f*_rn helpers are header functions compiled with contraction on)
    const float nnt = 1.0f - (dones[i] ? 1.0f : 0.0f);
    const float t1 = gamma * nv;
    const float t2 = t1 * nnt;
    const float t3 = rewards[i] + t2;
    const float delta = t3 - v;
    const float t4 = gl * nnt;
    const float t5 = t4 * last_adv;
    last_adv = delta + t5;
    adv[i] = last_adv;
    ret[i] = last_adv + v;
    nv = v;
  }
}

// ---------------------------------------------------------------------------
// ms_sample_masked: one wave per row; Gumbel-max over valid cells.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float uniform01(uint64_t seed, uint64_t counter, uint64_t row, uint64_t col) {
  const uint64_t h = splitmix64(seed ^ splitmix64(counter ^ splitmix64(row * 0x100000001B3ull + col)));
  // 24 random bits -> (0, 1)
  return ((float)(h >> 40) + 0.5f) * (1.0f / 16777216.0f);
}

// ---------------------------------------------------------------------------
// ms_dropout_masks: Dropout2d channel masks keyed by GLOBAL sample index.
// out[b][i][c] = (u(seed', counter, rows[i], b*C + c) >= p) / (1 - p), so a
// sample draws the same masks whichever rank (or minibatch position) holds it.
// One thread per 4 output channels (float4 store).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dropout(const int64_t* __restrict__ rows, int64_t N, int nblk, int C,
                                                 uint64_t seed, uint64_t counter, float p, float scale,
                                                 float* __restrict__ out) {
  const int C4 = C >> 2;
  const int64_t total = (int64_t)nblk * N * C4;
  const uint64_t s = splitmix64(seed ^ 0xD1B54A32D192ED03ull);  // domain-separated from k_sample
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total;
       q += (int64_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(q % C4);
    const int64_t bi = q / C4;
    const int64_t i = bi % N;
    const int b = (int)(bi / N);
    const uint64_t row = (uint64_t)rows[i];
    float4 v;
    float* vp = &v.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float u = uniform01(s, counter, row, (uint64_t)(b * C + 4 * c4 + j));
      vp[j] = u >= p ? scale : 0.f;
    }
    reinterpret_cast<float4*>(out)[q] = v;
  }
}

__global__ __launch_bounds__(256) void k_sample(const float* __restrict__ logits, const uint8_t* __restrict__ mask,
                                                int64_t N, int A, int64_t row_begin, uint64_t seed,
                                                uint64_t counter, int64_t* __restrict__ actions,
                                                float* __restrict__ logp) {
  const int lane = lane_id();
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
  if (row >= N) return;
  const float* lr = logits + row * A;
  const uint8_t* mr = mask + row * A;
  int any = 0;
  for (int i = lane; i < A; i += kWave) any |= mr[i] ? 1 : 0;
  const bool all_valid = __ballot(any) == 0ull;  // train_rl.py:166-168
  float mx = -INFINITY;
  for (int i = lane; i < A; i += kWave)
    if (all_valid || mr[i]) mx = fmaxf(mx, lr[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
  float se = 0.f;
  float best = -INFINITY;
  int best_i = 0x7fffffff;
  for (int i = lane; i < A; i += kWave) {
    if (all_valid || mr[i]) {
      const float l = lr[i];
      se += expf(l - mx);
      const float u = uniform01(seed, counter, (uint64_t)(row_begin + row), (uint64_t)i);
      const float gk = l - logf(-logf(u));
      if (gk > best || (gk == best && i < best_i)) {
        best = gk;
        best_i = i;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    se += __shfl_xor(se, off);
    const float ob = __shfl_xor(best, off);
    const int oi = __shfl_xor(best_i, off);
    if (ob > best || (ob == best && oi < best_i)) {
      best = ob;
      best_i = oi;
    }
  }
  if (lane == 0) {
    actions[row] = best_i;
    logp[row] = (lr[best_i] - mx) - logf(se);
  }
}

// the hipGetLastError tail of a launch: MS_OK, or "<where>: <hip error>" as ms_last_error()
int launched(const char* where) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return MS_OK;
  char msg[512];
  snprintf(msg, sizeof msg, "%s: %s", where, hipGetErrorString(e));
  return ms_internal_fail(MS_EHIP, msg);
}

}  // namespace

extern "C" {

int ms_gae(const float* rewards, const float* values, const uint8_t* dones, const float* last_values, int32_t T,
           int64_t N, float gamma, float gamma_lambda, float* adv, float* ret, void* stream) {
  if (!rewards || !values || !dones || !last_values || !adv || !ret || T <= 0 || N <= 0)
    return ms_internal_fail(MS_EINVAL, "ms_gae: bad argument");
  hipLaunchKernelGGL(k_gae, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rewards, values,
                     dones, last_values, (int)T, N, gamma, gamma_lambda, adv, ret);
  return launched("ms_gae launch");
}

int ms_sample_masked(const float* logits, const uint8_t* mask, int64_t N, int32_t A, int64_t row_begin,
                     uint64_t seed, uint64_t counter, int64_t* actions, float* logp, void* stream) {
  if (!logits || !mask || !actions || !logp || N <= 0 || A <= 0 || row_begin < 0)
    return ms_internal_fail(MS_EINVAL, "ms_sample_masked: bad argument");
  hipLaunchKernelGGL(k_sample, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, mask, N,
                     (int)A, row_begin, seed, counter, actions, logp);
  return launched("ms_sample_masked launch");
}

int ms_dropout_masks(const int64_t* rows, int64_t N, int32_t nblk, int32_t C, uint64_t seed, uint64_t counter,
                     float p, float* out, void* stream) {
  if (!rows || !out || N <= 0 || nblk <= 0 || C <= 0 || (C & 3) || !(p > 0.f && p < 1.f))
    return ms_internal_fail(MS_EINVAL, "ms_dropout_masks: bad argument");
  const int64_t total = (int64_t)nblk * N * (C / 4);
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 8192);
  hipLaunchKernelGGL(k_dropout, dim3(grid), dim3(256), 0, (hipStream_t)stream, rows, N, (int)nblk, (int)C, seed,
                     counter, p, 1.0f / (1.0f - p), out);
  return launched("ms_dropout_masks launch");
}

}  // extern "C"
