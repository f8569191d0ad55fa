// msbc.hip — the behaviour-cloning minibatch loss against expert targets and its backward as HIP
// passes (C ABI include/msbc.h), in the shape of msppo.hip: one wavefront owns a row, the row's A
// logits sit in registers (NQ = A / 64 per lane), the softmax statistics are wave reductions, and
// the per-row terms go to fixed-order partial sums.
//
//   k_bc_loss_fwd  per row of weight != 0: x = masked logits; max, log-sum-exp, entropy; the mean
//                  of log pi over the expert's best cells; whether the lowest-index argmax of x is
//                  one of them (ballots over 64-cell slices in ascending order). Per row of any
//                  weight: the pos-weighted BCE and the calibration error of the belief logits
//                  over the valid cells. Per-row (max, log-sum, entropy, n_best) go to the
//                  workspace for the backward (n_best = NaN marks a bad row); per-workgroup sums
//                  of the five terms and of the bad rows to partial rows.
//   k_bc_loss_fin  one workgroup: the partial rows summed in a fixed order, the normalisations of
//                  msbc.h, and the weighted loss.
//   k_bc_loss_bwd  per row: the gradient of sum_k gout[k] out[k]; 0 at masked cells and on rows
//                  of weight 0, which are not read.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include "../../include/msenv.h"
#include "../../include/mscnn.h"
#include "../../include/msbc.h"
#include "mscnn_common.h"

namespace {

using namespace mc;

constexpr int NTERM = 6;        // cross entropy, agreement, entropy, bce, calibration sums; bad rows
constexpr int PSTRIDE = 8;      // floats per partial row
constexpr int RSTRIDE = 4;      // floats per row statistics: max, log-sum, entropy, n_best (NaN: bad row)
constexpr int MAX_GRID = 2048;  // workgroups (4 rows in flight each); fixed, so sums never depend on the device
constexpr int MAX_A = 512;

inline int loss_grid(int64_t M) {
  const int64_t g = (M + 3) / 4;
  return (int)(g < MAX_GRID ? g : MAX_GRID);
}

// butterfly reductions: every lane ends with the same value (each step adds a pair in the same order)
__device__ __forceinline__ float bfly_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float bfly_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// pos_weight from the global (sum labels * valid, sum valid): (neg + 1e-6) / (pos + 1e-6)
__device__ __forceinline__ float pos_weight(const mc_bc_loss_args& a) {
  const float pos = a.counts[1], cnt = a.counts[2];
  return (cnt - pos + 1e-6f) / (pos + 1e-6f);
}

// world / sum of weights; 0 for an empty (or NaN) sum, so that the policy terms are 0, not NaN
__device__ __forceinline__ float row_norm(const mc_bc_loss_args& a) {
  const float c0 = a.counts[0];
  return c0 > 0.f ? a.world / c0 : 0.f;
}

template <int NQ>
__global__ __launch_bounds__(256) void k_bc_loss_fwd(mc_bc_loss_args a, float* __restrict__ part,
                                                      float* __restrict__ rows) {
  __shared__ float sp[4][NTERM];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int A = a.A;
  const float pw = a.mine ? pos_weight(a) : 1.0f;
  float acc[NTERM] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // lane 0: this wave's running sums, rows in order
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < a.M; r += (int64_t)gridDim.x * 4) {
    const float w = a.weight[r];
    float ce = 0.f, agree = 0.f, h = 0.f, bad = 0.f;
    if (w != 0.f) {
      const float* lr = a.logits + r * A;
      const uint8_t* mr = a.action_mask + r * A;
      const uint8_t* br = a.best + r * A;
      float x[NQ];
      bool bq[NQ];
      float mx = -INFINITY;
      bool on_masked = false;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int j = lane + 64 * q;
        x[q] = -INFINITY;
        bq[q] = false;
        if (j < A) {
          const bool legal = mr[j] != 0;
          x[q] = legal ? lr[j] : a.mask_fill;
          bq[q] = br[j] != 0;
          on_masked |= bq[q] && !legal;
        }
        mx = fmaxf(mx, x[q]);
      }
      mx = bfly_max(mx);
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        if (lane + 64 * q < A) s += expf(x[q] - mx);
      const float ls = logf(bfly_sum(s));
      float sb = 0.f;  // sum of log pi over the best cells
      int nb = 0, am = -1, am_best = 0;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if (lane + 64 * q < A) {
          const float lp = (x[q] - mx) - ls;
          h -= expf(lp) * lp;
          if (bq[q]) sb += lp;
        }
        const unsigned long long mb = __ballot(bq[q]);
        const unsigned long long me = __ballot(lane + 64 * q < A && x[q] == mx);
        nb += __popcll(mb);
        if (am < 0 && me) {  // the lowest index that attains the maximum
          am = __ffsll((long long)me) - 1;
          am_best = (int)((mb >> am) & 1ull);
        }
      }
      h = bfly_sum(h);
      sb = bfly_sum(sb);
      const bool is_bad = nb == 0 || __ballot(on_masked) != 0ull;
      ce = is_bad ? NAN : -(sb / (float)nb);
      agree = (float)am_best;
      bad = is_bad ? 1.f : 0.f;
      if (lane == 0) {
        float* rs = rows + r * RSTRIDE;
        rs[0] = mx;
        rs[1] = ls;
        rs[2] = h;
        rs[3] = is_bad ? NAN : (float)nb;
      }
    }
    float bce = 0.f, cal = 0.f;
    if (a.mine) {  // msppo's belief terms over the valid cells; the count and pos_weight are global
      const float* lm = a.mine + r * A;
      const float* yr = a.labels + r * A;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int j = lane + 64 * q;
        if (j < A && (!a.valid || a.valid[r * A + j])) {
          const float y = yr[j], lf = lm[j];
          const float lsig = fminf(lf, 0.f) - log1pf(expf(-fabsf(lf)));  // log sigmoid(lf)
          bce += (1.f - y) * lf - lsig * ((pw - 1.f) * y + 1.f);
          const float d = sigmoidf(lf) - y;
          cal += d * d;
        }
      }
      bce = bfly_sum(bce);
      cal = bfly_sum(cal);
    }
    if (lane == 0) {
      if (w != 0.f) {
        acc[0] += w * ce;
        acc[1] += w * agree;
        acc[2] += w * h;
      }
      acc[3] += bce;
      acc[4] += cal;
      acc[5] += bad;
    }
  }
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < NTERM; ++k) sp[wave][k] = acc[k];
  __syncthreads();
  if (threadIdx.x < PSTRIDE)
    part[(size_t)blockIdx.x * PSTRIDE + threadIdx.x] =
        threadIdx.x < NTERM ? (sp[0][threadIdx.x] + sp[1][threadIdx.x]) + (sp[2][threadIdx.x] + sp[3][threadIdx.x]) : 0.f;
}

__global__ __launch_bounds__(256) void k_bc_loss_fin(mc_bc_loss_args a, const float* __restrict__ part, int G,
                                                     float* __restrict__ out) {
  __shared__ float sm[NTERM][256];
  float s[NTERM] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int g = threadIdx.x; g < G; g += 256)
#pragma unroll
    for (int k = 0; k < NTERM; ++k) s[k] += part[(size_t)g * PSTRIDE + k];
#pragma unroll
  for (int k = 0; k < NTERM; ++k) sm[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
#pragma unroll
      for (int k = 0; k < NTERM; ++k) sm[k][threadIdx.x] += sm[k][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = row_norm(a);
    const bool any = norm != 0.f;  // an empty weight sum gives 0, not 0 * sum
    const float ce = any ? sm[0][0] * norm : 0.f, agree = any ? sm[1][0] * norm : 0.f;
    const float ent = any ? sm[2][0] * norm : 0.f;
    float bce = 0.f, cal = 0.f;
    if (a.mine) {
      const float scale = a.world / fmaxf(a.counts[2], 1.0f);  // empty valid set -> 0
      bce = sm[3][0] * scale;
      cal = sm[4][0] * scale;
    }
    float loss = ce - a.ent_coef * ent;
    if (a.mine && a.aux_mine_weight > 0.f) loss = loss + a.aux_mine_weight * bce;
    if (a.mine && a.aux_mine_calib_weight > 0.f) loss = loss + a.aux_mine_calib_weight * cal;
    out[0] = ce;
    out[1] = agree;
    out[2] = ent;
    out[3] = bce;
    out[4] = cal;
    out[5] = loss;
    out[6] = sm[5][0];  // bad rows (an exact count below 2^24)
    out[7] = 0.f;
  }
}

template <int NQ>
__global__ __launch_bounds__(256) void k_bc_loss_bwd(mc_bc_loss_args a, const float* __restrict__ gout,
                                                      const float* __restrict__ rows, float* __restrict__ dlogits,
                                                      float* __restrict__ dmine) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int A = a.A;
  // d loss / d out[k] folded into each term's coefficient (out[5] is the weighted sum of out[0], [2..4])
  const float g5 = gout[5];
  const float norm = row_norm(a);
  const float c_ce = (gout[0] + g5) * norm, c_ent = (gout[2] - g5 * a.ent_coef) * norm;
  const float c_bce = gout[3] + (a.aux_mine_weight > 0.f ? g5 * a.aux_mine_weight : 0.f);
  const float c_cal = gout[4] + (a.aux_mine_calib_weight > 0.f ? g5 * a.aux_mine_calib_weight : 0.f);
  const float pw = a.mine ? pos_weight(a) : 1.0f;
  const float scale = a.mine ? a.world / fmaxf(a.counts[2], 1.0f) : 0.f;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < a.M; r += (int64_t)gridDim.x * 4) {
    const float w = a.weight[r];
    float* dl = dlogits + r * A;
    if (w != 0.f && norm != 0.f) {
      const float* rs = rows + r * RSTRIDE;
      const float mx = rs[0], ls = rs[1], h = rs[2];
      const float nb = rs[3];
      const float inv_nb = 1.0f / nb;
      const float G = nb != nb ? NAN : c_ce * w, E = c_ent * w;  // a bad row: NaN at its legal cells
      const float* lr = a.logits + r * A;
      const uint8_t* mr = a.action_mask + r * A;
      const uint8_t* br = a.best + r * A;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int j = lane + 64 * q;
        if (j < A) {
          float d = 0.f;  // masked_fill's backward: 0 at masked cells
          if (mr[j]) {
            const float lp = (lr[j] - mx) - ls, p = expf(lp);
            // -(1 / n) sum_best log pi: p_j - [j in best] / n; entropy: dH/dx_j = -p_j (log p_j + H)
            d = G * (p - (br[j] ? inv_nb : 0.f)) - E * (p * (lp + h));
          }
          dl[j] = d;
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        if (lane + 64 * q < A) dl[lane + 64 * q] = 0.f;
    }
    if (a.mine) {
      const float* lm = a.mine + r * A;
      const float* yr = a.labels + r * A;
      float* dm = dmine + r * A;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int j = lane + 64 * q;
        if (j < A) {
          float d = 0.f;
          if (!a.valid || a.valid[r * A + j]) {
            const float y = yr[j], lf = lm[j], sg = sigmoidf(lf);
            // BCE with pos_weight: (pw y + 1 - y) sigmoid(x) - pw y per unit gradient; only when the
            // term has a coefficient. Calibration: 2 (s - y) s (1 - s)
            const float gb = c_bce != 0.f ? c_bce * scale * (((pw * y + 1.f - y) * sg) - pw * y) : 0.f;
            const float gs = c_cal * scale * (2.f * (sg - y)) * ((1.f - sg) * sg);
            d = gb + gs;
          }
          dm[j] = d;
        }
      }
    }
  }
}

bool args_ok(const mc_bc_loss_args* a, const char* what) {
  const char* bad = nullptr;
  if (!a) bad = "null args";
  else if (!a->logits || !a->action_mask || !a->best || !a->weight || !a->counts) bad = "null row tensor or counts";
  else if (a->M <= 0 || a->A <= 0 || a->A > MAX_A) bad = "M must be >= 1 and A in 1..512";
  else if (a->mine && !a->labels) bad = "mine logits need labels";
  if (bad) {
    snprintf(g_err, sizeof g_err, "%s: bad argument (%s)", what, bad);
    return false;
  }
  return true;
}

int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_err, sizeof g_err, "%s launch: %s", what, hipGetErrorString(e));
    return MS_EHIP;
  }
  return MS_OK;
}

}  // namespace

extern "C" {

int64_t mc_bc_loss_workspace(int64_t M) {
  if (M <= 0) return -1;
  return (int64_t)MAX_GRID * PSTRIDE + M * RSTRIDE;
}

int mc_bc_loss_fwd(const mc_bc_loss_args* a, float* out, float* work, int64_t work_floats, void* stream) {
  if (!args_ok(a, "mc_bc_loss_fwd")) return MS_EINVAL;
  if (!out || !work || work_floats < mc_bc_loss_workspace(a->M)) {
    snprintf(g_err, sizeof g_err, "mc_bc_loss_fwd: bad argument (out / workspace)");
    return MS_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  const int G = loss_grid(a->M);
  float* part = work;
  float* rows = work + (size_t)MAX_GRID * PSTRIDE;
  if (a->A <= 128) hipLaunchKernelGGL(k_bc_loss_fwd<2>, dim3(G), dim3(256), 0, s, *a, part, rows);
  else if (a->A <= 256) hipLaunchKernelGGL(k_bc_loss_fwd<4>, dim3(G), dim3(256), 0, s, *a, part, rows);
  else hipLaunchKernelGGL(k_bc_loss_fwd<8>, dim3(G), dim3(256), 0, s, *a, part, rows);
  if (int rc = launched("k_bc_loss_fwd")) return rc;
  hipLaunchKernelGGL(k_bc_loss_fin, dim3(1), dim3(256), 0, s, *a, part, G, out);
  return launched("k_bc_loss_fin");
}

int mc_bc_loss_bwd(const mc_bc_loss_args* a, const float* gout, const float* work, int64_t work_floats,
                   float* dlogits, float* dmine, void* stream) {
  if (!args_ok(a, "mc_bc_loss_bwd")) return MS_EINVAL;
  if (!gout || !work || work_floats < mc_bc_loss_workspace(a->M) || !dlogits || (a->mine && !dmine)) {
    snprintf(g_err, sizeof g_err, "mc_bc_loss_bwd: bad argument (gout / workspace / outputs)");
    return MS_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  const int G = loss_grid(a->M);
  const float* rows = work + (size_t)MAX_GRID * PSTRIDE;
  if (a->A <= 128) hipLaunchKernelGGL(k_bc_loss_bwd<2>, dim3(G), dim3(256), 0, s, *a, gout, rows, dlogits, dmine);
  else if (a->A <= 256) hipLaunchKernelGGL(k_bc_loss_bwd<4>, dim3(G), dim3(256), 0, s, *a, gout, rows, dlogits, dmine);
  else hipLaunchKernelGGL(k_bc_loss_bwd<8>, dim3(G), dim3(256), 0, s, *a, gout, rows, dlogits, dmine);
  return launched("k_bc_loss_bwd");
}

}  // extern "C"
