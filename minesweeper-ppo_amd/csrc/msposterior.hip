// Exact mine-probability posterior on device (include/msposterior.h, msposterior_labels.h): one
// wavefront per board.
//
// The board sits in LDS as row bitboards like k_avoid's (csrc/mssolve.hip), lane r owns row r
// for the row-parallel steps and lane l owns cells l, l + 64, ... for the cell-parallel ones.
//   1 frontier, closure   as k_avoid; the numbers stand in for the mine plane
//   2 consistency         every constraint must still be satisfiable after the closure
//   3 components          of the reduced system: min-label propagation over the free cells
//   4 counts              per component one query per lane ("variable q is a mine", lane 0 of the
//                         first chunk unconstrained): iterative depth-first search over 128-bit
//                         value strings; a leaf increments the lane's own histogram entry for
//                         its mine count (LDS, hist[k][lane]) and backtracks. No atomics.
//   5 combine             f64, fixed order: V[m] = C(U, R - m) with every component but j folded
//                         in (V[m] <- sum_s N_i[s] V[m + s], one m per lane) is the weight of a
//                         solution of j with m mines; all folded in, V[0] = Z.
// A board of two or more components runs the unconstrained queries of all components first (the
// weights of one need the counts of all others); the per-cell histograms never leave LDS.
// Every loop has a bound fixed before it starts: label and closure rounds by the frontier size,
// the search by the node budget. A board the search cannot finish is reported undecided.
//
// The counting stage too is chosen at compile time: k_posterior<*, true> (msposterior_grouped.h)
// searches over groups of equivalent cells (csrc/msposterior_grouped_device.h) with f64 counts
// in its own LDS layout (LdsG); the <*, false> instantiations compile to what they were.
// The output stage is chosen at compile time: k_posterior<false> writes the f64 posterior and its
// status (ms_posterior, ms_posterior_states); k_posterior<true> writes training targets in
// k_labels' layout (ms_posterior_labels): the posterior rounded to f32 where the search decided,
// the handle's own mine rows where it did not.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "../../include/msposterior.h"
#include "../../include/msposterior_grouped.h"
#include "../../include/msposterior_labels.h"
#include "msenv_internal.h"
#include "mssolve_device.h"
#include "msposterior_grouped_device.h"
#include "msposterior_host.h"

namespace {

constexpr int kWave = 64;
constexpr int kMaxCells = MS_AVOID_MAX_CELLS;
constexpr int kMaxVars = MS_AVOID_MAX_VARS;
constexpr uint32_t kNoLabel = 0xFFFFu;
constexpr uint16_t kNoCon = 0xFFFFu;

struct PostOut {
  uint8_t* status;
  double* prob;
  double* configs;
  int32_t* max_nodes;
  // ms_posterior_labels only (k_posterior<true>)
  float* labels;
  uint8_t* valid;
  uint8_t* source;
};

struct PostSrc {
  // a handle's packed planes (ms_posterior) ...
  const uint64_t* mine_words;
  const uint64_t* rev_words;
  const uint8_t* meta;
  int32_t meta_stride, flags_offset, NW;
  // ... or byte planes (ms_posterior_states)
  const uint8_t* rev_u8;
  const uint8_t* num_u8;
};

struct Lds {
  // fre: the safe plane during the closure, the free plane (frontier, undecided) after it
  uint64_t rev[kWave + 2], fr[kWave + 2], fre[kWave + 2], fm[kWave + 2];
  uint32_t hist[(kMaxVars + 1) * kWave];          // hist[k * 64 + lane]: the lane's solutions with k mines
  uint64_t cm_lo[kMaxCells], cm_hi[kMaxCells];    // a component's constraints over local variables
  double cu[kMaxCells + 1];                       // cu[r] = C(U, r)
  double V[kMaxCells + 1];
  double p[kMaxCells];
  uint32_t label[kMaxCells];                      // component label of a free cell = its smallest cell index
  uint32_t nj[kMaxCells + kMaxCells / 2];         // N_j[k] of every component, back to back
  uint16_t njoff[kMaxCells / 2 + 2];              // where component j's counts start; [ncomp] = their end
  uint16_t vcell[kMaxVars];                       // local variable -> cell
  uint16_t vcons[kMaxVars * 8];                   // local variable -> its constraints, one slot per direction
  uint8_t num[kMaxCells];                         // adjacent mines of a revealed cell
  int8_t ctarget[kMaxCells];
  uint8_t lvar[kMaxCells];                        // cell -> local variable of the component in hand
};

// The layout of the grouped instantiations (csrc/msposterior_grouped_device.h): f64 histograms
// and counts, a value byte per group, constraints as lists of groups; 61,808 B.
struct LdsG {
  uint64_t rev[kWave + 2], fr[kWave + 2], fre[kWave + 2], fm[kWave + 2];
  double hist[kSlabG];                            // hist[k * ql + lane]: the lane's weighted solutions with k mines
  uint64_t cgl[kMaxCells];                        // a constraint's groups, a byte each (0xFF: none)
  double cu[kMaxCells + 1];
  double V[kMaxCells + 1];
  double p[kMaxCells];
  double nj[kMaxCells + kMaxCells / 2];
  uint32_t cmult[kMaxCells];                      // the multiplicities of those groups, a nibble each
  uint32_t label[kMaxCells];
  uint16_t njoff[kMaxCells / 2 + 2];
  uint16_t vcell[kMaxVars];
  uint16_t vcons[kMaxVars * 8];                   // compacted by build_groups
  uint8_t val[kSlabG];                            // val[g * ql + lane]: the lane's value of group g
  uint8_t num[kMaxCells];
  int8_t ctarget[kMaxCells];
  uint8_t lvar[kMaxCells];
  uint8_t vgid[kMaxVars], gl[kMaxVars], gn[kMaxVars];  // variable -> group; group -> smallest variable, multiplicity
  uint8_t binom[88];                              // C(n, v), n, v <= 8
};
static_assert(sizeof(LdsG) <= 64 * 1024, "static LDS of a workgroup");

// V[m] <- sum_s N[s] V[m + s] for m in [0, len), N = L.nj[off .. off + cnt): lane-parallel over m,
// in place (a chunk reads only entries at or above its own, and reads them all before it writes)
template <class LdsT>
__device__ __forceinline__ void absorb(LdsT& L, int lane, int len, int off, int cnt) {
  for (int base = 0; base < len; base += kWave) {
    const int m = base + lane;
    double acc = 0.0;
    if (m < len)
      for (int s = 0; s < cnt && m + s < len; ++s) acc += (double)L.nj[off + s] * L.V[m + s];
    wave_sync();
    if (m < len) L.V[m] = acc;
    wave_sync();
  }
}

// cu[r] = C(n, r) for 0 <= r <= rmax (0 for r > n), by the multiplicative recurrence on lane 0
template <class LdsT>
__device__ __forceinline__ void binomial_row(LdsT& L, int lane, int n, int rmax) {
  if (lane == 0) {
    double c = n >= 0 ? 1.0 : 0.0;
    L.cu[0] = c;
    for (int r = 0; r < rmax; ++r) {
      c = r < n ? c * (double)(n - r) / (double)(r + 1) : 0.0;
      L.cu[r + 1] = c;
    }
  }
  wave_sync();
}

// V[m] = cu[top - m] for m in [0, top]
template <class LdsT>
__device__ __forceinline__ void load_tail(LdsT& L, int lane, int top) {
  for (int base = 0; base <= top; base += kWave) {
    const int m = base + lane;
    if (m <= top) L.V[m] = L.cu[top - m];
  }
  wave_sync();
}

template <bool kLabels, bool kGrouped>
__global__ __launch_bounds__(64) void k_posterior(PostSrc src, const uint8_t* __restrict__ live, int64_t n, int H,
                                                  int W, int M, int budget, PostOut o) {
  __shared__ std::conditional_t<kGrouped, LdsG, Lds> L;
  const int lane = lane_id();
  const int64_t env = blockIdx.x;
  if (env >= n) return;
  const int A = H * W;
  const bool handle = src.rev_words != nullptr;
  bool analysed = !live || live[env] != 0;
  const bool first_click = handle && (*(const uint32_t*)(src.meta + env * src.meta_stride + src.flags_offset) & 1u) != 0;
  if (handle) analysed = analysed && first_click;
  const bool too_big = A > kMaxCells;
  // the handle's rows of this lane (lane r holds row r; 0 for lane >= H)
  uint64_t rev = 0, mine = 0;
  auto load_rows = [&]() {
    const int rpw = 64 / W;
    const int w = lane / rpw;
    const int wc = w < src.NW ? w : src.NW - 1;
    const int sh = (lane - w * rpw) * W;
    const uint64_t keep = lane < H ? (1ull << W) - 1ull : 0ull;
    rev = (src.rev_words[env * src.NW + wc] >> sh) & keep;
    mine = (src.mine_words[env * src.NW + wc] >> sh) & keep;
  };

  uint8_t st = MS_AVOID_DECIDED;
  double Z = 0.0;
  int32_t max_nodes = 0;

  if (!analysed) {
    st = MS_AVOID_SKIPPED;
  } else if (too_big) {
    st = MS_AVOID_UNDECIDED;
    if constexpr (kLabels) load_rows();
  } else {
    // ---- load: lane r builds row r and the numbers of its cells
    if (handle) {
      load_rows();
      const uint64_t up = wave_shr1(mine) << 1, mid = mine << 1, dn = wave_shl1(mine) << 1;
      if (lane < H)
        for (int c = 0; c < W; ++c)
          L.num[lane * W + c] = (uint8_t)(__popcll((up >> c) & 7ull) + __popcll((mid >> c) & 5ull) +
                                          __popcll((dn >> c) & 7ull));
    } else if (lane < H) {
      const uint8_t* rp = src.rev_u8 + (env * H + lane) * W;
      const uint8_t* np = src.num_u8 + (env * H + lane) * W;
      for (int c = 0; c < W; ++c) {
        rev |= (uint64_t)(rp[c] != 0) << c;
        L.num[lane * W + c] = np[c];
      }
    }
    const int nrev = wave_sum(__popcll(rev));
    // ---- 1 frontier
    const uint64_t u = rev | wave_shr1(rev) | wave_shl1(rev);
    const uint64_t rowmask = lane < H ? (1ull << W) - 1ull : 0ull;
    const uint64_t fr = (u | (u << 1) | (u >> 1)) & ~rev & rowmask;
    L.rev[lane + 1] = rev << 1;
    L.fr[lane + 1] = fr << 1;
    L.fre[lane + 1] = 0;
    L.fm[lane + 1] = 0;
    if (lane == 0) {
      L.rev[0] = L.fr[0] = L.fre[0] = L.fm[0] = 0;
      L.rev[kWave + 1] = L.fr[kWave + 1] = L.fre[kWave + 1] = L.fm[kWave + 1] = 0;
    }
    for (int base = 0; base < A; base += kWave)
      if (base + lane < A) L.p[base + lane] = 0.0;
    if constexpr (kGrouped) binomial_table(L, lane);
    const int n_frontier = wave_sum(__popcll(fr));
    wave_sync();
    if (nrev == 0) {
      st = MS_AVOID_SKIPPED;  // nothing to condition on
    } else {
      uint64_t* const safe = L.fre;
      // ---- closure (k_avoid's, with the numbers as targets)
      for (int round = 0; round <= n_frontier; ++round) {
        bool changed = false;
        for (int base = 0; base < A; base += kWave) {  // unit rule
          const int i = base + lane;
          if (i < A) {
            const int r = i / W, c = i - r * W;
            if (cell_bit(L.rev, r, c)) {
              const uint32_t v = win9(L.fr, r, c) & ~16u, m = win9(L.fm, r, c);
              const uint32_t rem = v & ~win9(safe, r, c) & ~m;
              const int t = (int)L.num[i] - __popc(v & m), nr = __popc(rem);
              if (rem && t == 0) {
                or9(safe, r, c, rem);
                changed = true;
              } else if (rem && t == nr) {
                or9(L.fm, r, c, rem);
                changed = true;
              }
            }
          }
          wave_sync();
        }
        if (wave_any(changed)) continue;
        for (int base = 0; base < A; base += kWave) {  // strict-subset rule, a = this cell
          const int i = base + lane;
          if (i < A) {
            const int r = i / W, c = i - r * W;
            if (cell_bit(L.rev, r, c)) {
              const uint32_t va = win9(L.fr, r, c) & ~16u, ma = win9(L.fm, r, c);
              const uint32_t rema = va & ~win9(safe, r, c) & ~ma;
              const int ta = (int)L.num[i] - __popc(va & ma);
              if (rema) {
#pragma unroll
                for (int dr = -2; dr <= 2; ++dr) {
#pragma unroll
                  for (int dc = -2; dc <= 2; ++dc) {
                    if (dr == 0 && dc == 0) continue;
                    const int rb = r + dr, cb = c + dc;
                    if (rb < 0 || rb >= H || cb < 0 || cb >= W) continue;
                    if (!cell_bit(L.rev, rb, cb)) continue;
                    bool lost;
                    const uint32_t ainb = shift9(rema, dr, dc, lost);
                    if (lost) continue;
                    const uint32_t vb = win9(L.fr, rb, cb) & ~16u, mb = win9(L.fm, rb, cb);
                    const uint32_t remb = vb & ~win9(safe, rb, cb) & ~mb;
                    const uint32_t diff = remb & ~ainb;
                    if ((ainb & ~remb) || !diff) continue;
                    const int tb = (int)L.num[rb * W + cb] - __popc(vb & mb);
                    if (ta == tb) {
                      or9(safe, rb, cb, diff);
                      changed = true;
                    } else if (tb - ta == __popc(diff)) {
                      or9(L.fm, rb, cb, diff);
                      changed = true;
                    }
                  }
                }
              }
            }
          }
          wave_sync();
        }
        if (!wave_any(changed)) break;
      }
      // ---- 2 consistency: what the closure left must be satisfiable constraint by constraint
      bool bad = (safe[lane + 1] & L.fm[lane + 1]) != 0ull;
      for (int base = 0; base < A; base += kWave) {
        const int i = base + lane;
        if (i < A) {
          const int r = i / W, c = i - r * W;
          if (cell_bit(L.rev, r, c)) {
            const uint32_t v = win9(L.fr, r, c) & ~16u, m = win9(L.fm, r, c);
            const int t = (int)L.num[i] - __popc(v & m);
            if (t < 0 || t > __popc(v & ~win9(safe, r, c) & ~m)) bad = true;
          }
        }
      }
      const int R = M - wave_sum(__popcll(L.fm[lane + 1]));  // mines left for free and interior cells
      const int U = A - nrev - n_frontier;                   // interior cells
      bad = wave_any(bad) || R < 0;
      wave_sync();
      const uint64_t fre = L.fr[lane + 1] & ~safe[lane + 1] & ~L.fm[lane + 1];
      const int nfree = wave_sum(__popcll(fre));
      L.fre[lane + 1] = fre;  // from here on the plane holds the free cells
      wave_sync();
      bool undecided = false;
      int nodes_max = 0, ncomp = 0;
      if (!bad) {
        // ---- 3 components of the reduced system
        for (int base = 0; base < A; base += kWave) {
          const int i = base + lane;
          if (i < A) {
            const int r = i / W, c = i - r * W;
            L.label[i] = cell_bit(L.fre, r, c) ? (uint32_t)i : kNoLabel;
            if (cell_bit(L.fm, r, c)) L.p[i] = 1.0;
          }
        }
        wave_sync();
        for (int round = 0; round <= nfree; ++round) {
          bool changed = false;
          for (int base = 0; base < A; base += kWave) {
            const int i = base + lane;
            if (i < A) {
              const int r = i / W, c = i - r * W;
              const uint32_t v = cell_bit(L.rev, r, c) ? (win9(L.fre, r, c) & ~16u) : 0u;
              if (v) {
                uint32_t m = kNoLabel;
#pragma unroll
                for (int k = 0; k < 9; ++k)
                  if ((v >> k) & 1u) m = min(m, L.label[win_cell(i, W, k)]);
#pragma unroll
                for (int k = 0; k < 9; ++k)
                  if (((v >> k) & 1u) && L.label[win_cell(i, W, k)] > m) {
                    atomicMin(&L.label[win_cell(i, W, k)], m);
                    changed = true;
                  }
              }
            }
            wave_sync();
          }
          if (!wave_any(changed)) break;
        }
        int roots = 0;
        for (int base = 0; base < A; base += kWave) {
          const int i = base + lane;
          roots += i < A && L.label[i] == (uint32_t)i;
        }
        ncomp = wave_sum(roots);
        if (ncomp > kMaxCells / 2) undecided = true;  // cannot happen: a component has two cells or more
        binomial_row(L, lane, U, R);

        // ---- 4 counts and 5 combine, per component (roots in ascending cell order); a board of
        // several components first runs the unconstrained queries alone (pass 0)
        const bool multi = ncomp >= 2;
        if (ncomp == 0) Z = L.cu[R];
        for (int pass = multi ? 0 : 1; pass < 2 && !undecided; ++pass) {
          if (pass == 1 && multi) {
            load_tail(L, lane, R);
            for (int i = 0; i < ncomp; ++i) absorb(L, lane, R + 1, L.njoff[i], L.njoff[i + 1] - L.njoff[i]);
            Z = L.V[0];
            wave_sync();
            if (!(Z > 0.0)) break;
          }
          int j = 0, off = 0;
          for (int rbase = 0; rbase < A && !undecided; rbase += kWave) {
            const int ri = rbase + lane;
            uint64_t rootmask = ballot(ri < A && L.label[ri] == (uint32_t)ri);
            while (rootmask && !undecided) {
              const uint32_t root = (uint32_t)(rbase + __builtin_ctzll(rootmask));
              rootmask &= rootmask - 1ull;
              // search order: cell ascending
              int nv = 0;
              for (int base = 0; base < A; base += kWave) nv += __popcll(ballot(base + lane < A && L.label[base + lane] == root));
              if (nv > kMaxVars || off + nv + 1 > (int)(sizeof(L.nj) / sizeof(L.nj[0]))) {
                undecided = true;  // (the second cannot happen: a component has two cells or more)
                break;
              }
              int run = 0;
              for (int base = 0; base < A; base += kWave) {
                const int i = base + lane;
                const bool mine = i < A && L.label[i] == root;
                const uint64_t b = ballot(mine);
                const int rank = run + __popcll(b & lanes_below(lane));
                run += __popcll(b);
                if (i < A) L.lvar[i] = mine ? (uint8_t)rank : (uint8_t)0xFF;
                if (mine) {
                  L.vcell[rank] = (uint16_t)i;
#pragma unroll
                  for (int k = 0; k < 8; ++k) L.vcons[rank * 8 + k] = kNoCon;
                }
              }
              wave_sync();
              // the component's reduced constraints over local variables
              int nc = 0;
              for (int base = 0; base < A; base += kWave) {
                const int i = base + lane;
                uint32_t rem = 0;
                int t = 0;
                if (i < A) {
                  const int r = i / W, c = i - r * W;
                  if (cell_bit(L.rev, r, c)) {
                    const uint32_t v = win9(L.fre, r, c) & ~16u;
                    if (v && L.label[win_cell(i, W, __builtin_ctz(v))] == root) {
                      rem = v;
                      t = (int)L.num[i] - __popc(win9(L.fm, r, c));
                    }
                  }
                }
                const uint64_t b = ballot(rem != 0);
                if (rem) {
                  const int ci = nc + __popcll(b & lanes_below(lane));
                  Bits128 mask = {0, 0};
#pragma unroll
                  for (int k = 0; k < 9; ++k)
                    if ((rem >> k) & 1u) {
                      const int lv = L.lvar[win_cell(i, W, k)];
                      if (lv >= kMaxVars) continue;  // cannot happen: rem holds free cells of this component
                      const Bits128 bit = bit128(lv);
                      mask.lo |= bit.lo;
                      mask.hi |= bit.hi;
                      L.vcons[lv * 8 + (k < 4 ? k : k - 1)] = (uint16_t)ci;
                    }
                  if constexpr (!kGrouped) {  // (the grouped search keeps group lists: build_groups)
                    L.cm_lo[ci] = mask.lo;
                    L.cm_hi[ci] = mask.hi;
                  }
                  L.ctarget[ci] = (int8_t)t;
                }
                nc += __popcll(b);
              }
              wave_sync();
              int ng = 0;
              if constexpr (kGrouped) ng = build_groups(L, lane, A, W, root, nv);
              const bool first = pass == 0 || !multi;  // this pass produces N_j
              if (first) {
                L.njoff[j] = (uint16_t)off;
                L.njoff[j + 1] = (uint16_t)(off + nv + 1);
              }
              if (pass == 1) {  // V[k] = weight of a solution of this component with k mines
                load_tail(L, lane, R);
                for (int i = 0; i < ncomp; ++i)
                  if (i != j) absorb(L, lane, R + 1, L.njoff[i], L.njoff[i + 1] - L.njoff[i]);
              }
              // queries: lane 0 of the first chunk is unconstrained, the others "variable q is a mine"
              [[maybe_unused]] const int nq = pass == 0 ? 1 : nv + 1;
              if constexpr (kGrouped)  // one query per group instead, over the same N_j layout
                grouped_queries(L, lane, nv, ng, off, first, multi, pass, R, budget, nodes_max, undecided, Z);
              else  // (the loop keeps its indentation: its text is the enumerating kernel's, unchanged)
              for (int q0 = 0; q0 < nq && !undecided; q0 += kWave) {
                const bool active = q0 + lane < nq;
                const int q = q0 + lane - 1;
                const Bits128 qbit = active && q >= 0 ? bit128(q) : Bits128{0ull, 0ull};
                for (int k = 0; k <= nv; ++k) L.hist[k * kWave + lane] = 0;
                auto consistent = [&](int var, Bits128 val, Bits128 known) {
                  bool ok = true;
#pragma unroll
                  for (int k = 0; k < 8; ++k) {
                    const uint16_t ci = L.vcons[var * 8 + k];
                    if (ci == kNoCon) continue;
                    const uint64_t mlo = L.cm_lo[ci], mhi = L.cm_hi[ci];
                    const int t = L.ctarget[ci];
                    const int mines = __popcll(mlo & val.lo) + __popcll(mhi & val.hi);
                    const int unknown = __popcll(mlo & ~known.lo) + __popcll(mhi & ~known.hi);
                    if (mines > t || mines + unknown < t) ok = false;
                  }
                  return ok;
                };
                // res: 0 searching, 1 idle lane, 2 finished, 3 out of budget
                int res = active ? 0 : 1;
                Bits128 val = qbit;
                int nodes = active && q >= 0 ? 1 : 0;
                if (active && q >= 0 && !consistent(q, val, qbit)) res = 2;
                int d = q == 0 ? 1 : 0, x = 0;
                bool back = false;
                const int64_t iter_cap = 3 * (int64_t)budget + 2 * nv + 8;
                for (int64_t iter = 0; iter < iter_cap; ++iter) {
                  if (!wave_any(res == 0)) break;
                  if (res != 0) {
                    // this lane's query is finished; it idles until the wave's last one is
                  } else if (!back) {
                    if (d >= nv) {  // a leaf: count it and go on
                      L.hist[(__popcll(val.lo) + __popcll(val.hi)) * kWave + lane] += 1u;
                      back = true;
                    } else if (nodes >= budget) {
                      res = 3;
                    } else {
                      ++nodes;
                      const Bits128 dbit = bit128(d);
                      const Bits128 tryv = {val.lo | (x ? dbit.lo : 0ull), val.hi | (x ? dbit.hi : 0ull)};
                      Bits128 known = below128(d + 1);
                      known.lo |= qbit.lo;
                      known.hi |= qbit.hi;
                      if (consistent(d, tryv, known)) {
                        val = tryv;
                        d += 1;
                        if (d == q) d += 1;
                        x = 0;
                      } else if (x == 0) {
                        x = 1;
                      } else {
                        back = true;
                      }
                    }
                  } else {
                    d -= 1;
                    if (d == q) d -= 1;
                    if (d < 0) {
                      res = 2;
                    } else {
                      const Bits128 dbit = bit128(d);
                      const bool was1 = ((val.lo & dbit.lo) | (val.hi & dbit.hi)) != 0ull;
                      val.lo &= ~dbit.lo;
                      val.hi &= ~dbit.hi;
                      if (!was1) {
                        x = 1;
                        back = false;
                      }
                    }
                  }
                }
                if (res == 0) res = 3;
                nodes_max = max(nodes_max, nodes);
                if (wave_any(res == 3)) undecided = true;
                wave_sync();
                if (!undecided) {
                  if (first && q0 == 0) {  // lane 0's histogram is N_j
                    for (int base = 0; base <= nv; base += kWave)
                      if (base + lane <= nv) L.nj[off + base + lane] = L.hist[(base + lane) * kWave];
                    wave_sync();
                    if (!multi) {
                      double z = 0.0;
                      for (int k = 0; k <= nv && k <= R; ++k) z += (double)L.nj[off + k] * L.V[k];
                      Z = z;
                    }
                  }
                  if (pass == 1 && active && q >= 0) {
                    double acc = 0.0;
                    for (int k = 0; k <= nv && k <= R; ++k) acc += (double)L.hist[k * kWave + lane] * L.V[k];
                    L.p[L.vcell[q]] = acc;
                  }
                }
                wave_sync();
              }
              off += nv + 1;
              j += 1;
            }
          }
        }
        max_nodes = wave_max(nodes_max);
      }
      if (undecided) {
        st = MS_AVOID_UNDECIDED;
      } else if (bad || !(Z > 0.0)) {  // no layout reproduces the numbers
        st = MS_AVOID_UNDECIDED;
        max_nodes = 0;
      } else {
        // p of the free cells, and of the interior cells: every component folded into C(U-1, R-1-m)
        double pin = 0.0;
        if (U > 0 && R > 0) {
          wave_sync();
          binomial_row(L, lane, U - 1, R - 1);
          load_tail(L, lane, R - 1);
          for (int i = 0; i < ncomp; ++i) absorb(L, lane, R, L.njoff[i], L.njoff[i + 1] - L.njoff[i]);
          pin = fmin(L.V[0] / Z, 1.0);
        }
        for (int base = 0; base < A; base += kWave) {
          const int i = base + lane;
          if (i < A) {
            const int r = i / W, c = i - r * W;
            if (cell_bit(L.fre, r, c))
              L.p[i] = fmin(L.p[i] / Z, 1.0);  // a sure mine may round to 1 + 1 ulp
            else if (!cell_bit(L.rev, r, c) && !cell_bit(L.fr, r, c))
              L.p[i] = pin;
          }
        }
        wave_sync();
      }
    }
  }

  const bool decided = st == MS_AVOID_DECIDED;
  if constexpr (kLabels) {
    // k_labels' two planes (csrc/msenv.hip). Before the first click both are 0; a decided board's
    // labels are p rounded to f32 (p is 0 at revealed cells); any other board keeps its mine mask.
    wave_sync();  // every read of the planes below is done
    L.fm[lane] = mine;
    L.rev[lane] = rev;
    wave_sync();
    if (lane == 0) {
      if (o.source) o.source[env] = !first_click ? (uint8_t)0 : decided ? (uint8_t)1 : (uint8_t)2;
      if (o.max_nodes) o.max_nodes[env] = max_nodes;
    }
    for (int base = 0; base < A; base += kWave) {
      const int i = base + lane;
      if (i < A) {
        const int r = i / W, c = i - r * W;
        const uint32_t mb = (uint32_t)(L.fm[r] >> c) & 1u, rb = (uint32_t)(L.rev[r] >> c) & 1u;
        if (o.labels) o.labels[env * A + i] = !first_click ? 0.f : decided ? (float)L.p[i] : (float)mb;
        if (o.valid) o.valid[env * A + i] = first_click ? (uint8_t)(rb ^ 1u) : (uint8_t)0;
      }
    }
    return;
  }
  if (lane == 0) {
    if (o.status) o.status[env] = st;
    if (o.configs) o.configs[env] = decided ? Z : 0.0;
    if (o.max_nodes) o.max_nodes[env] = max_nodes;
  }
  if (o.prob)
    for (int base = 0; base < A; base += kWave) {
      const int i = base + lane;
      if (i < A) o.prob[env * A + i] = decided ? L.p[i] : 0.0;
    }
}

template <bool kLabels = false, bool kGrouped = false>
int launch(const PostSrc& src, const uint8_t* live, int64_t n, int H, int W, int M, int budget, const PostOut& o,
           void* stream, const char* who) {
  hipLaunchKernelGGL((k_posterior<kLabels, kGrouped>), dim3((unsigned)n), dim3(kWave), 0, (hipStream_t)stream, src, live, n, H, W, M,
                     budget, o);
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return MS_OK;
  char msg[256];
  snprintf(msg, sizeof msg, "%s launch: %s", who, hipGetErrorString(e));
  return ms_internal_fail(MS_EHIP, msg);
}

bool budget_ok(int32_t b) { return b >= 1 && b <= (1 << 30); }

PostSrc handle_src(const ms_board_view& v) {
  PostSrc src = {};
  src.mine_words = v.mine_words;
  src.rev_words = v.rev_words;
  src.meta = v.meta;
  src.meta_stride = v.meta_stride;
  src.flags_offset = v.flags_offset;
  src.NW = v.NW;
  return src;
}

int fail(const char* who, const char* what) {
  char msg[160];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return ms_internal_fail(MS_EINVAL, msg);
}

// The entry points of msposterior.h / msposterior_labels.h (kGrouped = false) and of
// msposterior_grouped.h (true): one body each, `who` names the entry point in messages.
template <bool kGrouped>
int posterior_impl(const char* who, ms_handle* h, const uint8_t* live, uint8_t* status, double* prob, double* configs,
                   int32_t* max_nodes, void* stream) {
  if (!h) return fail(who, "null handle");
  ms_board_view v;
  ms_internal_board_view(h, &v);
  const PostOut o = {status, prob, configs, max_nodes, nullptr, nullptr, nullptr};
  const int budget = *v.posterior_budget ? *v.posterior_budget : MS_POSTERIOR_DEFAULT_BUDGET;
  return launch<false, kGrouped>(handle_src(v), live, v.n, v.H, v.W, v.mine_count, budget, o, stream, who);
}

template <bool kGrouped>
int labels_impl(const char* who, ms_handle* h, int32_t budget, float* labels, uint8_t* valid, uint8_t* source,
                int32_t* max_nodes, void* stream) {
  if (!h) return fail(who, "null handle");
  if (!budget_ok(budget)) return fail(who, "need 1 <= budget <= 2^30");
  ms_board_view v;
  ms_internal_board_view(h, &v);
  const PostOut o = {nullptr, nullptr, nullptr, max_nodes, labels, valid, source};
  return launch<true, kGrouped>(handle_src(v), nullptr, v.n, v.H, v.W, v.mine_count, budget, o, stream, who);
}

template <bool kGrouped>
int states_impl(const char* who, const uint8_t* revealed, const uint8_t* number, int32_t mine_count, const uint8_t* live,
                int64_t n, int32_t H, int32_t W, int32_t budget, uint8_t* status, double* prob, double* configs,
                int32_t* max_nodes, void* stream) {
  if (!revealed || !number) return fail(who, "null revealed or number");
  if (n <= 0 || n > 0x7fffffffll) return fail(who, "need 1 <= n < 2^31");
  if (H < 1 || H > 64 || W < 1 || W > 62)
    return fail(who, "need 1<=H<=64, 1<=W<=62");
  if (mine_count < 0 || mine_count > H * W)
    return fail(who, "need 0 <= mine_count <= H*W");
  if (!budget_ok(budget)) return fail(who, "need 1 <= budget <= 2^30");
  PostSrc src = {};
  src.rev_u8 = revealed;
  src.num_u8 = number;
  const PostOut o = {status, prob, configs, max_nodes, nullptr, nullptr, nullptr};
  return launch<false, kGrouped>(src, live, n, H, W, mine_count, budget, o, stream, who);
}

template <bool kGrouped>
int host_impl(const char* who, const uint8_t* revealed, const uint8_t* number, int32_t mine_count, const uint8_t* live,
              int64_t n, int32_t H, int32_t W, int64_t host_budget, uint8_t* status, double* prob, double* configs,
              int32_t* max_nodes) {
  if (!revealed || !number) return fail(who, "null revealed or number");
  if (n <= 0) return fail(who, "need n >= 1");
  if (H < 1 || W < 1 || (int64_t)H * W > (1 << 20))
    return fail(who, "need H, W >= 1 and H*W <= 2^20");
  if (mine_count < 0 || mine_count > H * W)
    return fail(who, "need 0 <= mine_count <= H*W");
  if (host_budget < 0) return fail(who, "need host_budget >= 0");
  const int64_t A = (int64_t)H * W;
  int rc = MS_OK;
  for (int64_t e = 0; e < n; ++e) {
    double* pe = prob ? prob + e * A : nullptr;
    msposterior::Result R;
    if (live && !live[e]) {
      if (pe) std::fill(pe, pe + A, 0.0);
    } else {
      R = kGrouped ? msposterior::analyze_grouped(revealed + e * A, number + e * A, H, W, mine_count, host_budget, pe)
                   : msposterior::analyze(revealed + e * A, number + e * A, H, W, mine_count, host_budget, pe);
    }
    if (R.status == msposterior::kInconsistent) {
      char msg[160];
      snprintf(msg, sizeof msg, "%s: board %lld is inconsistent (no layout of %d mines reproduces its numbers)", who,
               (long long)e, (int)mine_count);
      rc = ms_internal_fail(MS_EINVAL, msg);
      R.status = msposterior::kUndecided;
      R.max_nodes = 0;
      if (pe) std::fill(pe, pe + A, 0.0);
    }
    if (status) status[e] = (uint8_t)R.status;
    if (configs) configs[e] = R.status == msposterior::kDecided ? R.configs : 0.0;
    if (max_nodes) max_nodes[e] = R.max_nodes;
  }
  return rc;
}

}  // namespace

extern "C" {

int ms_posterior_set_budget(ms_handle* h, int32_t nodes) {
  if (!h) return ms_internal_fail(MS_EINVAL, "ms_posterior_set_budget: null handle");
  if (!budget_ok(nodes)) return ms_internal_fail(MS_EINVAL, "ms_posterior_set_budget: need 1 <= nodes <= 2^30");
  ms_board_view v;
  ms_internal_board_view(h, &v);
  *v.posterior_budget = nodes;
  return MS_OK;
}

int ms_posterior(ms_handle* h, const uint8_t* live, uint8_t* status, double* prob, double* configs,
                 int32_t* max_nodes, void* stream) {
  return posterior_impl<false>("ms_posterior", h, live, status, prob, configs, max_nodes, stream);
}

int ms_posterior_grouped(ms_handle* h, const uint8_t* live, uint8_t* status, double* prob, double* configs,
                         int32_t* max_nodes, void* stream) {
  return posterior_impl<true>("ms_posterior_grouped", h, live, status, prob, configs, max_nodes, stream);
}

int ms_posterior_labels(ms_handle* h, int32_t budget, float* labels, uint8_t* valid, uint8_t* source,
                        int32_t* max_nodes, void* stream) {
  return labels_impl<false>("ms_posterior_labels", h, budget, labels, valid, source, max_nodes, stream);
}

int ms_posterior_labels_grouped(ms_handle* h, int32_t budget, float* labels, uint8_t* valid, uint8_t* source,
                                int32_t* max_nodes, void* stream) {
  return labels_impl<true>("ms_posterior_labels_grouped", h, budget, labels, valid, source, max_nodes, stream);
}

int ms_posterior_states(const uint8_t* revealed, const uint8_t* number, int32_t mine_count, const uint8_t* live,
                        int64_t n, int32_t H, int32_t W, int32_t budget, uint8_t* status, double* prob,
                        double* configs, int32_t* max_nodes, void* stream) {
  return states_impl<false>("ms_posterior_states", revealed, number, mine_count, live, n, H, W, budget, status, prob,
                            configs, max_nodes, stream);
}

int ms_posterior_states_grouped(const uint8_t* revealed, const uint8_t* number, int32_t mine_count,
                                const uint8_t* live, int64_t n, int32_t H, int32_t W, int32_t budget,
                                uint8_t* status, double* prob, double* configs, int32_t* max_nodes, void* stream) {
  return states_impl<true>("ms_posterior_states_grouped", revealed, number, mine_count, live, n, H, W, budget, status,
                           prob, configs, max_nodes, stream);
}

int ms_posterior_host(const uint8_t* revealed, const uint8_t* number, int32_t mine_count, const uint8_t* live,
                      int64_t n, int32_t H, int32_t W, int64_t host_budget, uint8_t* status, double* prob,
                      double* configs, int32_t* max_nodes) {
  return host_impl<false>("ms_posterior_host", revealed, number, mine_count, live, n, H, W, host_budget, status, prob,
                          configs, max_nodes);
}

int ms_posterior_host_grouped(const uint8_t* revealed, const uint8_t* number, int32_t mine_count,
                              const uint8_t* live, int64_t n, int32_t H, int32_t W, int64_t host_budget,
                              uint8_t* status, double* prob, double* configs, int32_t* max_nodes) {
  return host_impl<true>("ms_posterior_host_grouped", revealed, number, mine_count, live, n, H, W, host_budget, status,
                         prob, configs, max_nodes);
}

}  // extern "C"
