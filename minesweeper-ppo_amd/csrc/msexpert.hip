// msexpert.hip — expert policy targets from an exact posterior result (C ABI include/msexpert.h).
//
//   k_expert  one wavefront per board, four boards per workgroup. Lane l owns the cells
//             l, l + 64, ... (at most 8 of them, held in registers). The f64 minimum over the
//             hidden cells is a butterfly of lane exchanges; the size of the best set and its
//             lowest cell come from one ballot per 64-cell slice (slices in ascending order, so
//             the first set bit of the first non-empty ballot is the lowest index). Comparisons
//             and one f64 -> f32 conversion only: bitwise what msexpert_host.h computes.
//             No LDS, no atomics; every output is written by exactly one lane.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include "../../include/msexpert.h"
#include "msenv_internal.h"
#include "msexpert_host.h"

namespace {

constexpr int kWave = 64;
constexpr int kBoardsPerBlock = 4;
constexpr int kMaxQ = MS_AVOID_MAX_CELLS / kWave;  // 64-cell slices of the largest board
static_assert(kMaxQ * kWave == MS_AVOID_MAX_CELLS, "whole slices");

struct ExpertOut {
  uint8_t* best;
  int64_t* action;
  uint8_t* kind;
  int32_t* n_best;
  float* labels;
};

__global__ __launch_bounds__(kWave* kBoardsPerBlock) void k_expert(const uint8_t* __restrict__ status,
                                                                    const double* __restrict__ prob,
                                                                    const uint8_t* __restrict__ hidden, int64_t n,
                                                                    int A, ExpertOut o) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t env = (int64_t)blockIdx.x * kBoardsPerBlock + (threadIdx.x >> 6);
  if (env >= n) return;  // whole waves leave: the ballots below see full waves only
  const bool decided = status[env] == MS_AVOID_DECIDED;
  const double* pr = prob + env * A;
  const uint8_t* hr = hidden + env * A;
  double p[kMaxQ];
  bool hid[kMaxQ];
  double pmin = INFINITY;
#pragma unroll
  for (int q = 0; q < kMaxQ; ++q) {
    const int c = lane + kWave * q;
    hid[q] = decided && c < A && hr[c] != 0;
    p[q] = hid[q] ? pr[c] : 0.0;
    if (hid[q] && p[q] < pmin) pmin = p[q];
  }
#pragma unroll
  for (int s = kWave / 2; s > 0; s >>= 1) {
    const double other = __shfl_xor(pmin, s);
    if (other < pmin) pmin = other;
  }
  int64_t act = -1;
  int nb = 0;
#pragma unroll
  for (int q = 0; q < kMaxQ; ++q) {
    const int c = lane + kWave * q;
    const bool b = hid[q] && p[q] == pmin;
    const unsigned long long m = __ballot(b);
    if (act < 0 && m) act = kWave * q + __ffsll((long long)m) - 1;
    nb += __popcll(m);
    if (c < A) {
      if (o.best) o.best[env * A + c] = b ? 1 : 0;
      if (o.labels) o.labels[env * A + c] = hid[q] ? (float)p[q] : 0.f;
    }
  }
  if (lane == 0) {
    if (o.action) o.action[env] = act;
    if (o.n_best) o.n_best[env] = nb;
    if (o.kind) o.kind[env] = nb == 0 ? MS_EXPERT_NONE : (pmin == 0.0 ? MS_EXPERT_SAFE : MS_EXPERT_GUESS);
  }
}

int fail(const char* who, const char* what) {
  char msg[160];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return ms_internal_fail(MS_EINVAL, msg);
}

int args_bad(const char* who, const uint8_t* status, const double* prob, const uint8_t* hidden, int64_t n, int32_t A) {
  if (!status || !prob || !hidden) return fail(who, "null status, prob or hidden");
  if (n <= 0 || n > 0x7fffffffll) return fail(who, "need 1 <= n < 2^31");
  if (A < 1 || A > MS_AVOID_MAX_CELLS) return fail(who, "need 1 <= A <= 512");
  return MS_OK;
}

}  // namespace

extern "C" {

int ms_expert_targets(const uint8_t* status, const double* prob, const uint8_t* hidden, int64_t n, int32_t A,
                      uint8_t* best, int64_t* action, uint8_t* kind, int32_t* n_best, float* labels, void* stream) {
  if (int rc = args_bad("ms_expert_targets", status, prob, hidden, n, A)) return rc;
  const ExpertOut o = {best, action, kind, n_best, labels};
  const unsigned grid = (unsigned)((n + kBoardsPerBlock - 1) / kBoardsPerBlock);
  hipLaunchKernelGGL(k_expert, dim3(grid), dim3(kWave * kBoardsPerBlock), 0, (hipStream_t)stream, status, prob, hidden,
                     n, (int)A, o);
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return MS_OK;
  char msg[256];
  snprintf(msg, sizeof msg, "ms_expert_targets launch: %s", hipGetErrorString(e));
  return ms_internal_fail(MS_EHIP, msg);
}

int ms_expert_targets_host(const uint8_t* status, const double* prob, const uint8_t* hidden, int64_t n, int32_t A,
                           uint8_t* best, int64_t* action, uint8_t* kind, int32_t* n_best, float* labels) {
  if (int rc = args_bad("ms_expert_targets_host", status, prob, hidden, n, A)) return rc;
  for (int64_t e = 0; e < n; ++e) {
    int64_t act;
    int32_t nb;
    const int k = msexpert::board_targets(status[e], prob + e * A, hidden + e * A, A, best ? best + e * A : nullptr,
                                          labels ? labels + e * A : nullptr, &act, &nb);
    if (action) action[e] = act;
    if (n_best) n_best[e] = nb;
    if (kind) kind[e] = (uint8_t)k;
  }
  return MS_OK;
}

}  // extern "C"
