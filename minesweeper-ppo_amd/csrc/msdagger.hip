// msdagger.hip — the action mix of on-policy imitation (C ABI include/msdagger.h).
//
//   k_dagger  k_expert's shape: one wavefront per row, four rows per workgroup, lane l owns the
//             cells l, l + 64, ... Per row two keyed coins decide who plays: a uniform legal
//             click, the learner (greedy arg-max or a Gumbel-max sample of its logits) or the
//             teacher's action. The uniform action and the learner's sample restate k_sample's
//             key (csrc/msrollout.hip) operation for operation, so they are bit for bit what
//             ms_sample_masked returns; the keys of a row are computed only where the row's
//             outcome needs them (both conditions are wave-uniform). Reductions are butterflies
//             of lane exchanges. No LDS, no atomics, no scratch; every output element is written
//             by lane 0 of its row with a plain vector store.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include "../../include/msdagger.h"
#include "msenv_internal.h"
#include "msenv_pcg.h"

namespace {

constexpr int kWave = 64;
constexpr int kRowsPerBlock = 4;
constexpr int kNone = 0x7fffffff;  // "no cell yet" of the arg-max reductions; never stored

// csrc/msrollout.hip's uniform01, restated so that file's kernels stay as they are: 24 hash bits
// -> (0, 1), exact in f32
__device__ __forceinline__ float uniform01(uint64_t seed, uint64_t counter, uint64_t row, uint64_t col) {
  const uint64_t h = splitmix64(seed ^ splitmix64(counter ^ splitmix64(row * 0x100000001B3ull + col)));
  return ((float)(h >> 40) + 0.5f) * (1.0f / 16777216.0f);
}

// (key, cell) of the wave's best: the larger key, the lower cell among equal keys
__device__ __forceinline__ void wave_argmax(float& best, int& best_i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ob = __shfl_xor(best, off);
    const int oi = __shfl_xor(best_i, off);
    if (ob > best || (ob == best && oi < best_i)) {
      best = ob;
      best_i = oi;
    }
  }
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
  return v;
}

// k_sample's Gumbel-max over the legal cells of one row: the same key, the same comparison. With
// lr == nullptr the logits are zero (the uniform action). kNone when every legal key is NaN.
__device__ __forceinline__ int gumbel_argmax(const float* __restrict__ lr, const uint8_t* __restrict__ mr,
                                             bool all_valid, int A, int lane, uint64_t seed, uint64_t counter,
                                             uint64_t R) {
  float best = -INFINITY;
  int best_i = kNone;
  for (int i = lane; i < A; i += kWave) {
    if (all_valid || mr[i]) {
      const float l = lr ? lr[i] : 0.f;
      const float u = uniform01(seed, counter, R, (uint64_t)i);
      const float gk = l - logf(-logf(u));
      if (gk > best || (gk == best && i < best_i)) {
        best = gk;
        best_i = i;
      }
    }
  }
  wave_argmax(best, best_i);
  return best_i;
}

struct DaggerOut {
  int64_t* action;
  uint8_t* source;
  int64_t* learner_action;
  uint8_t* agree;
};

__global__ __launch_bounds__(kWave* kRowsPerBlock) void k_dagger(const float* __restrict__ logits,
                                                                  const uint8_t* __restrict__ mask,
                                                                  const uint8_t* __restrict__ best,
                                                                  const int64_t* __restrict__ expert_action,
                                                                  const uint8_t* __restrict__ kind, int64_t n, int A,
                                                                  int64_t row_begin, uint64_t seed, uint64_t counter,
                                                                  float beta, float explore, int mode, DaggerOut o) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= n) return;  // whole waves leave: the ballot and the exchanges below see full waves only
  const uint64_t R = (uint64_t)(row_begin + row);
  const uint8_t* mr = mask + row * A;
  int first = kNone;  // this lane's lowest legal cell
  for (int i = lane; i < A; i += kWave)
    if (first == kNone && mr[i]) first = i;
  const bool all_valid = __ballot(first != kNone) == 0ull;
  const int lowest = all_valid ? 0 : wave_min(first);  // the row's lowest legal cell

  const float cb = uniform01(splitmix64(seed ^ MS_DAGGER_C_BETA), counter, R, 0);
  const float ce = uniform01(splitmix64(seed ^ MS_DAGGER_C_EXPLORE), counter, R, 0);
  const bool has_target = kind[row] != MS_EXPERT_NONE;
  int src;
  if (ce < explore)
    src = MS_DAGGER_SRC_UNIFORM;
  else if (cb >= beta)
    src = MS_DAGGER_SRC_LEARNER;
  else
    src = has_target ? MS_DAGGER_SRC_EXPERT : MS_DAGGER_SRC_UNIFORM;

  int l = -1;
  if (logits) {
    const float* lr = logits + row * A;
    if (mode == MS_DAGGER_SAMPLE) {
      l = gumbel_argmax(lr, mr, all_valid, A, lane, splitmix64(seed ^ MS_DAGGER_C_LEARNER), counter, R);
    } else {
      // only a logit above -inf takes the lead, so NaN and -inf cells never do
      float bl = -INFINITY;
      l = kNone;
      for (int i = lane; i < A; i += kWave) {
        if (all_valid || mr[i]) {
          const float v = lr[i];
          if (v > bl) {
            bl = v;
            l = i;
          }
        }
      }
      wave_argmax(bl, l);
    }
    if (l == kNone) l = lowest;
  }

  int64_t act;
  if (src == MS_DAGGER_SRC_LEARNER) {
    act = l;
  } else if (src == MS_DAGGER_SRC_EXPERT) {
    act = expert_action[row];
  } else {
    const int u = gumbel_argmax(nullptr, mr, all_valid, A, lane, seed, counter, R);
    act = u == kNone ? lowest : u;  // a key on zero logits is finite: kNone cannot happen
  }
  if (lane == 0) {
    o.action[row] = act;
    if (o.source) o.source[row] = (uint8_t)src;
    if (o.learner_action) o.learner_action[row] = l;
    if (o.agree) o.agree[row] = (logits && has_target && best[row * A + l] != 0) ? 1 : 0;
  }
}

int fail(const char* what) {
  char msg[160];
  snprintf(msg, sizeof msg, "ms_dagger_act: %s", what);
  return ms_internal_fail(MS_EINVAL, msg);
}

}  // namespace

extern "C" {

int ms_dagger_act(const float* logits, const uint8_t* mask, const uint8_t* best, const int64_t* expert_action,
                  const uint8_t* kind, int64_t n, int32_t A, int64_t row_begin, uint64_t seed, uint64_t counter,
                  float beta, float explore, int32_t mode, int64_t* action, uint8_t* source,
                  int64_t* learner_action, uint8_t* agree, void* stream) {
  if (!mask || !expert_action || !kind || !action) return fail("null mask, expert_action, kind or action");
  if (n <= 0 || n > 0x7fffffffll) return fail("need 1 <= n < 2^31");
  if (A < 1 || A > MS_DAGGER_MAX_CELLS) return fail("need 1 <= A <= 3968");
  if (row_begin < 0) return fail("need row_begin >= 0");
  if (!(beta >= 0.f && beta <= 1.f)) return fail("beta must lie in [0, 1]");
  if (!(explore >= 0.f && explore <= 1.f)) return fail("explore must lie in [0, 1]");
  if (mode != MS_DAGGER_GREEDY && mode != MS_DAGGER_SAMPLE)
    return fail("mode must be MS_DAGGER_GREEDY or MS_DAGGER_SAMPLE");
  if (!logits && beta < 1.f) return fail("null logits need beta >= 1");
  if (logits && agree && !best) return fail("agree needs best");
  const DaggerOut o = {action, source, learner_action, agree};
  const unsigned grid = (unsigned)((n + kRowsPerBlock - 1) / kRowsPerBlock);
  hipLaunchKernelGGL(k_dagger, dim3(grid), dim3(kWave * kRowsPerBlock), 0, (hipStream_t)stream, logits, mask, best,
                     expert_action, kind, n, (int)A, row_begin, seed, counter, beta, explore, (int)mode, o);
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return MS_OK;
  char msg[256];
  snprintf(msg, sizeof msg, "ms_dagger_act launch: %s", hipGetErrorString(e));
  return ms_internal_fail(MS_EHIP, msg);
}

}  // extern "C"
