// mslookahead.hip — the two-guess lookahead of the exact-posterior player (C ABI
// include/mslookahead.h), around the unchanged ms_posterior_states* entry points.
//
//   k_la_flag    one wavefront per board, four per workgroup, in the shape of k_expert: lane l owns
//                the cells l, l + 64, ... in registers; the f64 minimum over the hidden cells is a
//                butterfly. Lane 0 writes 1 into slot[] for a guess board, 0 otherwise.
//   k_la_scan    one workgroup: an exclusive prefix sum of those flags in board order (a chunk per
//                thread, the chunk sums scanned in LDS), rewritten in place as slot numbers. This
//                is what makes the slot order deterministic without an atomic.
//   k_la_expand  one wavefront per board again. K rounds of a wave-wide arg-min over
//                (prob, cell index) pick the candidates in order: each lane's eligible cells stay in
//                its registers, the reduction is lane exchanges, no LDS. For each candidate the
//                wave writes the (at most nine) boards S(c, v), cell l + 64 q by lane l. The waves
//                numbered count .. cap - 1 pad the unused slots.
//   k_la_score   one wavefront per (board, candidate): for each decided outcome row, the number of
//                hidden cells, whether one has p = 0, and the smallest p, by ballots and a
//                butterfly; then the sums of the rule with every f64 operation rounded on its own.
//   k_la_choose  one lane per board: the scored candidate of largest score.
// No atomics; every output element is written by exactly one lane with a plain vector store.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include <vector>

#include "../../include/mslookahead.h"
#include "msenv_internal.h"
#include "mslookahead_host.h"

// A second copy of the host solver and the host lookahead, under other namespace names, with
// every function of it compiled for a CPU with fused multiply-add (see host_board_fma below). The
// standard headers are already included above, so nothing outside the two headers is affected.
#if defined(__x86_64__) && defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#define MS_LOOKAHEAD_HOST_FMA 1
#pragma clang attribute push(__attribute__((target("fma"))), apply_to = function)
#undef MSPOSTERIOR_HOST_H
#undef MSLOOKAHEAD_HOST_H
#define msposterior msposterior_fma
#define mslookahead mslookahead_fma
#include "mslookahead_host.h"
#undef msposterior
#undef mslookahead
#pragma clang attribute pop
#endif

namespace {

constexpr int kWave = 64;
constexpr int kBoardsPerBlock = 4;
constexpr int kMaxQ = MS_AVOID_MAX_CELLS / kWave;  // 64-cell slices of the largest board
constexpr int kScanThreads = 1024;
constexpr int kNone = 0x7fffffff;
static_assert(kMaxQ * kWave == MS_AVOID_MAX_CELLS, "whole slices");
static_assert(MS_LOOKAHEAD_MAX_K <= kWave && MS_LOOKAHEAD_OUTCOMES <= kWave, "one lane per candidate / outcome");
static_assert(mslookahead::kMaxK == MS_LOOKAHEAD_MAX_K && mslookahead::kOutcomes == MS_LOOKAHEAD_OUTCOMES &&
                  mslookahead::kRtol == MS_LOOKAHEAD_SCORED_RTOL,
              "the host twin's constants");

__device__ inline double wave_min(double x) {
#pragma unroll
  for (int s = kWave / 2; s > 0; s >>= 1) {
    const double other = __shfl_xor(x, s);
    if (other < x) x = other;
  }
  return x;
}

__global__ __launch_bounds__(kWave* kBoardsPerBlock) void k_la_flag(const uint8_t* __restrict__ status,
                                                                     const double* __restrict__ prob,
                                                                     const uint8_t* __restrict__ revealed, int64_t n,
                                                                     int A, int32_t* __restrict__ slot) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t env = (int64_t)blockIdx.x * kBoardsPerBlock + (threadIdx.x >> 6);
  if (env >= n) return;  // whole waves leave
  const bool decided = status[env] == MS_AVOID_DECIDED;
  double pmin = INFINITY;
#pragma unroll
  for (int q = 0; q < kMaxQ; ++q) {
    const int c = lane + kWave * q;
    if (decided && c < A && revealed[env * A + c] == 0) {
      const double p = prob[env * A + c];
      if (p < pmin) pmin = p;
    }
  }
  pmin = wave_min(pmin);
  // no hidden cell: pmin stays +inf; all-NaN rows (no ms_posterior* call writes one) too
  if (lane == 0) slot[env] = (decided && pmin > 0.0 && pmin < INFINITY) ? 1 : 0;
}

__global__ __launch_bounds__(kScanThreads) void k_la_scan(int32_t* __restrict__ slot, int64_t n, int64_t cap,
                                                          int32_t* __restrict__ count) {
  __shared__ int32_t part[kScanThreads];
  const int t = threadIdx.x;
  const int64_t chunk = (n + kScanThreads - 1) / kScanThreads;
  const int64_t lo = t * chunk < n ? t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
  int32_t sum = 0;
  for (int64_t i = lo; i < hi; ++i) sum += slot[i];
  part[t] = sum;
  __syncthreads();
  for (int s = 1; s < kScanThreads; s <<= 1) {  // inclusive scan of the chunk sums
    const int32_t add = t >= s ? part[t - s] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int64_t next = part[t] - sum;  // guess boards before this chunk
  for (int64_t i = lo; i < hi; ++i) {
    const bool g = slot[i] != 0;
    slot[i] = g && next < cap ? (int32_t)next : -1;
    next += g;
  }
  if (t == kScanThreads - 1) count[0] = part[t];
}

struct ExpandOut {
  int32_t* cand;
  uint8_t* revealed2;
  uint8_t* number2;
  uint8_t* live2;
};

__global__ __launch_bounds__(kWave* kBoardsPerBlock) void k_la_expand(const double* __restrict__ prob,
                                                                       const uint8_t* __restrict__ revealed,
                                                                       const uint8_t* __restrict__ number, int64_t n,
                                                                       int W, int A, int K, double margin, int64_t cap,
                                                                       const int32_t* __restrict__ slot,
                                                                       const int32_t* __restrict__ count, ExpandOut o) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t w = (int64_t)blockIdx.x * kBoardsPerBlock + (threadIdx.x >> 6);
  const int rows = K * MS_LOOKAHEAD_OUTCOMES;
  // the unused slots: no candidate, no live row
  if (w < cap && w >= (int64_t)count[0]) {
    if (lane < K) o.cand[w * K + lane] = -1;
    for (int i = lane; i < rows; i += kWave) o.live2[w * rows + i] = 0;
  }
  if (w >= n) return;
  const int s = slot[w];
  if (s < 0) return;  // whole waves leave: the ballots below see full waves only
  const double* pr = prob + w * A;
  double p[kMaxQ];
  bool el[kMaxQ];
  uint8_t rv[kMaxQ], nm[kMaxQ];
  int row[kMaxQ], col[kMaxQ];
  double pmin = INFINITY;
#pragma unroll
  for (int q = 0; q < kMaxQ; ++q) {
    const int c = lane + kWave * q;
    const bool in = c < A;
    rv[q] = in ? (uint8_t)(revealed[w * A + c] != 0) : (uint8_t)1;
    nm[q] = in ? number[w * A + c] : (uint8_t)0;
    p[q] = (in && !rv[q]) ? pr[c] : INFINITY;
    row[q] = c / W;
    col[q] = c - row[q] * W;
    if (p[q] < pmin) pmin = p[q];
  }
  pmin = wave_min(pmin);
  const double thr = pmin + margin;
#pragma unroll
  for (int q = 0; q < kMaxQ; ++q) el[q] = !rv[q] && p[q] <= thr;
  int mine = -1;  // lane k keeps candidate k
  for (int k = 0; k < K; ++k) {
    // the smallest (prob, index) still eligible: ascending q is ascending index within a lane
    double bp = INFINITY;
    int bi = kNone;
#pragma unroll
    for (int q = 0; q < kMaxQ; ++q)
      if (el[q] && (bi == kNone || p[q] < bp)) {
        bp = p[q];
        bi = lane + kWave * q;
      }
#pragma unroll
    for (int sft = kWave / 2; sft > 0; sft >>= 1) {
      const double op = __shfl_xor(bp, sft);
      const int oi = __shfl_xor(bi, sft);
      if (oi != kNone && (bi == kNone || op < bp || (op == bp && oi < bi))) {
        bp = op;
        bi = oi;
      }
    }
    const int c = bi == kNone ? -1 : bi;
    if (lane == k) mine = c;
    const int64_t r0 = ((int64_t)s * K + k) * MS_LOOKAHEAD_OUTCOMES;
    if (c < 0) {
      if (lane < MS_LOOKAHEAD_OUTCOMES) o.live2[r0 + lane] = 0;
      continue;
    }
    const int cr = c / W, cc = c - cr * W;
    int hidden_nb = 0;
#pragma unroll
    for (int q = 0; q < kMaxQ; ++q) {
      const int cell = lane + kWave * q;
      if (cell == c) el[q] = false;
      const int dr = row[q] - cr, dc = col[q] - cc;
      const bool nb = !rv[q] && cell != c && dr >= -1 && dr <= 1 && dc >= -1 && dc <= 1;
      hidden_nb += __popcll(__ballot(nb));
    }
    if (lane < MS_LOOKAHEAD_OUTCOMES) o.live2[r0 + lane] = lane <= hidden_nb ? 1 : 0;
    for (int v = 0; v < MS_LOOKAHEAD_OUTCOMES && v <= hidden_nb; ++v) {
      uint8_t* r2 = o.revealed2 + (r0 + v) * A;
      uint8_t* n2 = o.number2 + (r0 + v) * A;
#pragma unroll
      for (int q = 0; q < kMaxQ; ++q) {
        const int cell = lane + kWave * q;
        if (cell < A) {
          r2[cell] = cell == c ? (uint8_t)1 : rv[q];
          n2[cell] = cell == c ? (uint8_t)v : nm[q];
        }
      }
    }
  }
  if (lane < K) o.cand[(int64_t)s * K + lane] = mine;
}

__global__ __launch_bounds__(kWave* kBoardsPerBlock) void k_la_score(
    const int32_t* __restrict__ slot, const int32_t* __restrict__ cand, const double* __restrict__ prob,
    const double* __restrict__ configs, const uint8_t* __restrict__ status2, const double* __restrict__ prob2,
    const double* __restrict__ configs2, const uint8_t* __restrict__ revealed2, int M, int64_t n, int A, int K,
    int64_t cap, double* __restrict__ score) {
#pragma clang fp contract(off)  // every product, sum and difference below rounds on its own, as on the host
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t g = (int64_t)blockIdx.x * kBoardsPerBlock + (threadIdx.x >> 6);
  const int64_t w = g / K;
  const int k = (int)(g - w * K);
  // an unused slot has no candidate 0
  if (w < cap && cand[w * K] < 0 && lane == 0) score[w * K + k] = NAN;
  if (w >= n) return;
  const int s = slot[w];
  if (s < 0) return;
  const int64_t sk = (int64_t)s * K + k;
  const int c = cand[sk];
  if (c < 0) {
    if (lane == 0) score[sk] = NAN;
    return;
  }
  const double pc = prob[w * A + c], Z = configs[w];
  double sum_z = 0.0, sum_zt = 0.0;
  for (int v = 0; v < MS_LOOKAHEAD_OUTCOMES; ++v) {
    const int64_t r = sk * MS_LOOKAHEAD_OUTCOMES + v;
    if (status2[r] != MS_AVOID_DECIDED) continue;  // not live, cannot occur, or out of budget
    const double zv = configs2[r];
    int hidden = 0;
    bool safe = false;
    double pm = INFINITY;
#pragma unroll
    for (int q = 0; q < kMaxQ; ++q) {
      const int cell = lane + kWave * q;
      const bool h = cell < A && revealed2[r * A + cell] == 0;
      const double pv = h ? prob2[r * A + cell] : INFINITY;
      hidden += __popcll(__ballot(h));
      const unsigned long long zeros = __ballot(h && pv == 0.0);
      safe = safe || zeros != 0;
      if (pv < pm) pm = pv;
    }
    pm = wave_min(pm);
    double t = 1.0;
    if (hidden != M && !safe) t = 1.0 - pm;
    const double zt = zv * t;
    sum_zt = sum_zt + zt;
    sum_z = sum_z + zv;
  }
  const double q1 = 1.0 - pc;
  const double want = Z * q1;
  const double diff = fabs(sum_z - want);
  const double tol = MS_LOOKAHEAD_SCORED_RTOL * want;
  const double sc = sum_zt / Z;
  if (lane == 0) score[sk] = diff <= tol ? sc : NAN;
}

struct ChooseOut {
  int64_t* action;
  int32_t* n_scored;
  uint8_t* changed;
};

__global__ __launch_bounds__(256) void k_la_choose(const int32_t* __restrict__ slot, const int32_t* __restrict__ cand,
                                                   const double* __restrict__ score, int64_t n, int K, ChooseOut o) {
  const int64_t env = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n) return;
  const int s = slot[env];
  int64_t act = -1;
  int ns = 0, best = -1;
  if (s >= 0) {
    double bs = 0.0;
    for (int k = 0; k < K; ++k) {
      const double v = score[(int64_t)s * K + k];
      if (v != v) continue;  // NaN: unscored or padding
      ns += 1;
      if (best < 0 || v > bs) {
        best = k;
        bs = v;
      }
    }
    act = cand[(int64_t)s * K + (best < 0 ? 0 : best)];
  }
  o.action[env] = act;
  o.n_scored[env] = ns;
  o.changed[env] = best > 0 ? 1 : 0;
}

int fail(const char* who, const char* what) {
  char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return ms_internal_fail(MS_EINVAL, msg);
}

int shape_bad(const char* who, int64_t n, int32_t H, int32_t W, int32_t K, int64_t cap, int64_t n_max) {
  if (n <= 0 || n > n_max) return fail(who, n_max == 0x7fffffffll ? "need 1 <= n < 2^31" : "need 1 <= n < 2^27");
  if (H < 1 || W < 1 || (int64_t)H * W > MS_AVOID_MAX_CELLS) return fail(who, "need H, W >= 1 and H*W <= 512");
  if (K < 1 || K > MS_LOOKAHEAD_MAX_K) return fail(who, "need 1 <= K <= 16");
  if (cap < 1 || cap > 0x7fffffffll / (MS_LOOKAHEAD_MAX_K * MS_LOOKAHEAD_OUTCOMES))
    return fail(who, "need 1 <= cap and cap*K*9 < 2^31");
  return MS_OK;
}

bool margin_ok(double m) { return m >= 0.0 && m <= 1.0; }  // false for NaN

int launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return MS_OK;
  char msg[256];
  snprintf(msg, sizeof msg, "%s launch: %s", who, hipGetErrorString(e));
  return ms_internal_fail(MS_EHIP, msg);
}

unsigned blocks(int64_t waves) { return (unsigned)((waves + kBoardsPerBlock - 1) / kBoardsPerBlock); }

// The device compiler contracts the posterior kernel's `acc += count * weight` into fused
// multiply-adds; the host compiler has no such instruction to use by default, so the host solver's
// Z and p differ from the device's in the last bits wherever a product is not exact (the two are
// compared to 1e-12, tests/test_posterior_gpu.py). The twin's scores would then differ from the
// device's in the last bits too, and a tie between two candidates could fall the other way. So the
// twin runs the copy of the host solver that is compiled for a CPU with fused multiply-add (the
// same source, the same operation order, now the same roundings) whenever the CPU has it, and the
// plain one otherwise.
struct HostBoardArgs {
  const double* prob;
  double Z;
  const uint8_t *revealed, *number;
  int H, W, M;
  double pmin;
  int K;
  double margin;
  int64_t budget;
  bool grouped;
  int32_t* cand;
  double* score;
  int64_t* action;
  int32_t* n_scored;
  uint8_t* changed;
};

void host_board_plain(const HostBoardArgs& a, mslookahead::Scratch& s) {
  mslookahead::board(a.prob, a.Z, a.revealed, a.number, a.H, a.W, a.M, a.pmin, a.K, a.margin, a.budget, a.grouped, s,
                     a.cand, a.score, a.action, a.n_scored, a.changed);
}

#ifdef MS_LOOKAHEAD_HOST_FMA
__attribute__((target("fma"))) void host_board_fma(const HostBoardArgs& a, mslookahead::Scratch&) {
  mslookahead_fma::Scratch s;
  mslookahead_fma::board(a.prob, a.Z, a.revealed, a.number, a.H, a.W, a.M, a.pmin, a.K, a.margin, a.budget, a.grouped,
                         s, a.cand, a.score, a.action, a.n_scored, a.changed);
}
#endif

}  // namespace

extern "C" {

int ms_lookahead_expand(const uint8_t* status, const double* prob, const uint8_t* revealed, const uint8_t* number,
                        int64_t n, int32_t H, int32_t W, int32_t K, double margin, int64_t cap, int32_t* slot,
                        int32_t* count, int32_t* cand, uint8_t* revealed2, uint8_t* number2, uint8_t* live2,
                        void* stream) {
  const char* who = "ms_lookahead_expand";
  if (!status || !prob || !revealed || !number) return fail(who, "null status, prob, revealed or number");
  if (!slot || !count || !cand || !revealed2 || !number2 || !live2) return fail(who, "null output");
  if (int rc = shape_bad(who, n, H, W, K, cap, 0x7fffffffll)) return rc;
  if (!margin_ok(margin)) return fail(who, "need 0 <= margin <= 1");
  const int A = H * W;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_la_flag, dim3(blocks(n)), dim3(kWave * kBoardsPerBlock), 0, st, status, prob, revealed, n, A,
                     slot);
  hipLaunchKernelGGL(k_la_scan, dim3(1), dim3(kScanThreads), 0, st, slot, n, cap, count);
  const ExpandOut o = {cand, revealed2, number2, live2};
  hipLaunchKernelGGL(k_la_expand, dim3(blocks(n > cap ? n : cap)), dim3(kWave * kBoardsPerBlock), 0, st, prob,
                     revealed, number, n, (int)W, A, (int)K, margin, cap, slot, count, o);
  return launched(who);
}

int ms_lookahead_score(const int32_t* slot, const int32_t* cand, const double* prob, const double* configs,
                       const uint8_t* status2, const double* prob2, const double* configs2,
                       const uint8_t* revealed2, int32_t mine_count, int64_t n, int32_t H, int32_t W, int32_t K,
                       int64_t cap, int64_t* action, double* score, int32_t* n_scored, uint8_t* changed,
                       void* stream) {
  const char* who = "ms_lookahead_score";
  if (!slot || !cand || !prob || !configs) return fail(who, "null slot, cand, prob or configs");
  if (!status2 || !prob2 || !configs2 || !revealed2) return fail(who, "null status2, prob2, configs2 or revealed2");
  if (!action || !score || !n_scored || !changed) return fail(who, "null output");
  if (int rc = shape_bad(who, n, H, W, K, cap, 0x7fffffffll / MS_LOOKAHEAD_MAX_K)) return rc;
  if (mine_count < 0 || mine_count > H * W) return fail(who, "need 0 <= mine_count <= H*W");
  const int A = H * W;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_la_score, dim3(blocks((n > cap ? n : cap) * K)), dim3(kWave * kBoardsPerBlock), 0, st, slot,
                     cand, prob, configs, status2, prob2, configs2, revealed2, (int)mine_count, n, A, (int)K, cap,
                     score);
  const ChooseOut o = {action, n_scored, changed};
  hipLaunchKernelGGL(k_la_choose, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, slot, cand, score, n, (int)K,
                     o);
  return launched(who);
}

int ms_lookahead_host(const uint8_t* status, const double* prob, const double* configs, const uint8_t* revealed,
                      const uint8_t* number, int32_t mine_count, int64_t n, int32_t H, int32_t W, int32_t K,
                      double margin, int64_t cap, int64_t budget, int32_t grouped, int32_t* slot, int32_t* count,
                      int32_t* cand, int64_t* action, double* score, int32_t* n_scored, uint8_t* changed) {
  const char* who = "ms_lookahead_host";
  if (!status || !prob || !configs || !revealed || !number)
    return fail(who, "null status, prob, configs, revealed or number");
  if (!slot || !count || !cand || !action || !score || !n_scored || !changed) return fail(who, "null output");
  if (int rc = shape_bad(who, n, H, W, K, cap, 0x7fffffffll)) return rc;
  if (!margin_ok(margin)) return fail(who, "need 0 <= margin <= 1");
  if (mine_count < 0 || mine_count > H * W) return fail(who, "need 0 <= mine_count <= H*W");
  if (budget < 0) return fail(who, "need budget >= 0");
  const int A = H * W;
  mslookahead::Scratch scratch;
  void (*host_board)(const HostBoardArgs&, mslookahead::Scratch&) = host_board_plain;
#ifdef MS_LOOKAHEAD_HOST_FMA
  if (__builtin_cpu_supports("fma")) host_board = host_board_fma;
#endif
  int64_t guesses = 0;
  for (int64_t e = 0; e < n; ++e) {
    double pmin;
    const bool guess = mslookahead::guess_board(status[e], prob + e * A, revealed + e * A, A, &pmin);
    slot[e] = -1;
    action[e] = -1;
    n_scored[e] = 0;
    changed[e] = 0;
    if (!guess) continue;
    const int64_t s = guesses++;
    if (s >= cap) continue;
    slot[e] = (int32_t)s;
    const HostBoardArgs a = {prob + e * A, configs[e], revealed + e * A, number + e * A, H, W, mine_count, pmin, K,
                             margin, budget, grouped != 0, cand + s * K, score + s * K, action + e, n_scored + e,
                             changed + e};
    host_board(a, scratch);
  }
  for (int64_t s = guesses < cap ? guesses : cap; s < cap; ++s)
    for (int k = 0; k < K; ++k) {
      cand[s * K + k] = -1;
      score[s * K + k] = NAN;
    }
  count[0] = (int32_t)guesses;
  return MS_OK;
}

}  // extern "C"
