// The grouped counting stage of k_posterior<*, true> (include/msposterior_grouped.h): the groups
// of a component and the depth-first search over them. Internal to csrc/msposterior.hip, which
// owns the LDS layout (LdsG) and everything around the counting; every function here is inlined
// into the kernel.
//
// A lane's value string is one byte per group in LDS (val[g * ql + lane]); a constraint keeps the
// list of its groups as eight bytes (cgl) and their multiplicities as eight nibbles (cmult), so a
// constraint's sums are one walk over at most eight group ids. The leaf weight prod C(n_g, v_g)
// is recomputed at the leaf, in ascending g, from a 9 x 9 table in LDS: no running product has
// to be undone on the way back, and no division happens.
//
// The histograms are f64 (hist[k * ql + lane]). They share a fixed slab: ql, the queries searched
// at a time, is 64 while a component has at most kRows64 - 1 free cells, 32 up to twice that and
// 16 beyond (up to MS_AVOID_MAX_VARS), so that (free cells + 1) * ql entries always fit.
#ifndef MSPOSTERIOR_GROUPED_DEVICE_H
#define MSPOSTERIOR_GROUPED_DEVICE_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/mssolve.h"
#include "mssolve_device.h"

namespace {

constexpr int kRows64 = 49;                // histogram rows (free cells + 1) at 64 queries a time
constexpr int kSlabG = kRows64 * 64;       // entries of hist, and bytes of val
constexpr uint16_t kNoConG = 0xFFFFu;
static_assert(2 * kRows64 * 32 <= kSlabG && (MS_AVOID_MAX_VARS + 1) * 16 <= kSlabG, "hist rows fit at every ql");
static_assert((kRows64 - 1) * 64 <= kSlabG && (2 * kRows64 - 1) * 32 <= kSlabG && MS_AVOID_MAX_VARS * 16 <= kSlabG,
              "a value byte per group fits at every ql");

// binom[n * 9 + v] = C(n, v), 0 <= v, n <= 8 (0 for v > n): at most 70
template <class LdsT>
__device__ __forceinline__ void binomial_table(LdsT& L, int lane) {
  for (int i = lane; i < 81; i += 64) {
    const int n = i / 9, v = i - n * 9;
    int c = v <= n ? 1 : 0;
    for (int k = 0; k < v && v <= n; ++k) c = c * (n - k) / (k + 1);
    L.binom[i] = (uint8_t)c;
  }
}

// Groups of the component in hand (label == root; lvar, vcell, vcons and ctarget are built, vcons
// with one slot per direction): compacts every variable's constraint list, joins the variables
// whose lists are equal, numbers the groups by their smallest variable and rewrites every
// constraint as a list of groups. Returns the number of groups; afterwards
//   vgid[v] group of variable v, gl[g] its smallest variable, gn[g] its multiplicity,
//   vcons[gl[g] * 8 ..] the group's constraints (kNoConG-terminated), cgl / cmult per constraint.
template <class LdsT>
__device__ __forceinline__ int build_groups(LdsT& L, int lane, int A, int W, uint32_t root, int nv) {
  // a variable's slots are in descending constraint order, so equal sets compact to equal lists
  for (int v = lane; v < nv; v += 64) {
    int m = 0;
    for (int k = 0; k < 8; ++k) {
      const uint16_t c = L.vcons[v * 8 + k];
      if (c != kNoConG) L.vcons[v * 8 + m++] = c;
    }
    for (; m < 8; ++m) L.vcons[v * 8 + m] = kNoConG;
  }
  wave_sync();
  int ng = 0;
  int lead[2], cnt[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int v = h * 64 + lane;
    lead[h] = v;
    cnt[h] = 0;
    if (v < nv)
      for (int u = 0; u < nv; ++u) {
        bool same = true;
#pragma unroll
        for (int k = 0; k < 8; ++k) same = same && L.vcons[u * 8 + k] == L.vcons[v * 8 + k];
        if (same) {
          cnt[h] += 1;
          if (u < lead[h]) lead[h] = u;
        }
      }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int v = h * 64 + lane;
    const bool leader = v < nv && lead[h] == v;
    const uint64_t b = ballot(leader);
    if (leader) {
      const int g = ng + __popcll(b & lanes_below(lane));
      L.vgid[v] = (uint8_t)g;
      L.gl[g] = (uint8_t)v;
      L.gn[g] = (uint8_t)cnt[h];
    }
    ng += __popcll(b);
  }
  wave_sync();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int v = h * 64 + lane;
    if (v < nv && lead[h] != v) L.vgid[v] = L.vgid[lead[h]];
  }
  wave_sync();
  // the constraints again, in the order that numbered them, as lists of groups
  int nc = 0;
  for (int base = 0; base < A; base += 64) {
    const int i = base + lane;
    uint32_t rem = 0;
    if (i < A) {
      const int r = i / W, c = i - r * W;
      if (cell_bit(L.rev, r, c)) {
        const uint32_t v = win9(L.fre, r, c) & ~16u;
        if (v && L.label[win_cell(i, W, __builtin_ctz(v))] == root) rem = v;
      }
    }
    const uint64_t b = ballot(rem != 0);
    if (rem) {
      const int ci = nc + __popcll(b & lanes_below(lane));
      uint64_t list = ~0ull;
      uint32_t mult = 0;
      int m = 0;
#pragma unroll
      for (int k = 0; k < 9; ++k)
        if ((rem >> k) & 1u) {
          const int lv = L.lvar[win_cell(i, W, k)];
          if (lv >= MS_AVOID_MAX_VARS) continue;  // cannot happen: rem holds free cells of this component
          const uint32_t g = L.vgid[lv];
          bool seen = false;
          for (int s = 0; s < m; ++s) seen = seen || (uint32_t)((list >> (8 * s)) & 0xFFull) == g;
          if (!seen && m < 8) {
            list = (list & ~(0xFFull << (8 * m))) | ((uint64_t)g << (8 * m));
            mult |= (uint32_t)L.gn[g] << (4 * m);
            m += 1;
          }
        }
      L.cgl[ci] = list;
      L.cmult[ci] = mult;
    }
    nc += __popcll(b);
  }
  wave_sync();
  return ng;
}

// The queries of the component in hand: lane 0 of the first chunk is unconstrained, the others
// "the smallest cell of group q is a mine". Mirrors the enumerating query loop of k_posterior
// around another search; V holds the weights of pass 1.
template <class LdsT>
__device__ __forceinline__ void grouped_queries(LdsT& L, int lane, int nv, int ng, int off, bool first, bool multi,
                                                int pass, int R, int budget, int& nodes_max, bool& undecided,
                                                double& Z) {
  const int rows = nv + 1;
  const int ql = rows <= kRows64 ? 64 : rows <= 2 * kRows64 ? 32 : 16;
  const int nq = pass == 0 ? 1 : ng + 1;
  for (int q0 = 0; q0 < nq && !undecided; q0 += ql) {
    const bool active = lane < ql && q0 + lane < nq;
    const int q = active ? q0 + lane - 1 : -1;
    if (lane < ql) {
      for (int k = 0; k <= nv; ++k) L.hist[k * ql + lane] = 0.0;
      for (int g = 0; g < ng; ++g) L.val[g * ql + lane] = 0;
    }
    const int skip = q >= 0 && L.gn[q] == 1 ? q : -1;  // nothing left of q to search
    auto open_cells = [&](int g) { return (int)L.gn[g] - (g == q ? 1 : 0); };
    // the constraints of group cg with the groups below d assigned and group d taking x
    auto consistent = [&](int cg, int d, int x) {
      bool ok = true;
      const int lv = L.gl[cg];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint16_t ci = L.vcons[lv * 8 + k];
        if (ci == kNoConG) continue;
        const uint64_t list = L.cgl[ci];
        const uint32_t mult = L.cmult[ci];
        int t = L.ctarget[ci], mines = 0, unknown = 0;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const int g = (int)((list >> (8 * s)) & 0xFFull);
          if (g == 0xFF) continue;
          int n = (int)((mult >> (4 * s)) & 15u);
          if (g == q) {
            n -= 1;
            t -= 1;
          }
          if (g < d)
            mines += L.val[g * ql + lane];
          else if (g == d)
            mines += x;
          else
            unknown += n;
        }
        if (mines > t || mines + unknown < t) ok = false;
      }
      return ok;
    };
    // res: 0 searching, 1 idle lane, 2 finished, 3 out of budget
    int res = active ? 0 : 1;
    int nodes = q >= 0 ? 1 : 0, total = q >= 0 ? 1 : 0;
    if (q >= 0 && !consistent(q, -1, 0)) res = 2;
    int d = skip == 0 ? 1 : 0, x = 0;
    bool back = false;
    const int64_t iter_cap = 3 * (int64_t)budget + 2 * ng + 8;
    for (int64_t iter = 0; iter < iter_cap; ++iter) {
      if (!wave_any(res == 0)) break;
      if (res != 0) {
        // this lane's query is finished; it idles until the wave's last one is
      } else if (!back) {
        if (d >= ng) {  // a leaf: weigh it and go on
          double w = 1.0;
          for (int g = 0; g < ng; ++g) w *= (double)L.binom[open_cells(g) * 9 + L.val[g * ql + lane]];
          L.hist[total * ql + lane] += w;
          back = true;
        } else if (nodes >= budget) {
          res = 3;
        } else {
          ++nodes;
          if (consistent(d, d, x)) {
            L.val[d * ql + lane] = (uint8_t)x;
            total += x;
            d += 1;
            if (d == skip) d += 1;
            x = 0;
          } else if (x < open_cells(d)) {
            x += 1;
          } else {
            back = true;
          }
        }
      } else {
        d -= 1;
        if (d == skip) d -= 1;
        if (d < 0) {
          res = 2;
        } else {
          const int was = L.val[d * ql + lane];
          L.val[d * ql + lane] = 0;
          total -= was;
          if (was < open_cells(d)) {
            x = was + 1;
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
        for (int base = 0; base <= nv; base += 64)
          if (base + lane <= nv) L.nj[off + base + lane] = L.hist[(base + lane) * ql];
        wave_sync();
        if (!multi) {
          double z = 0.0;
          for (int k = 0; k <= nv && k <= R; ++k) z += L.nj[off + k] * L.V[k];
          Z = z;
        }
      }
      if (pass == 1 && q >= 0) {
        double acc = 0.0;
        for (int k = 0; k <= nv && k <= R; ++k) acc += L.hist[k * ql + lane] * L.V[k];
        for (int v = 0; v < nv; ++v)  // every cell of the group: they are symmetric
          if (L.vgid[v] == q) L.p[L.vcell[v]] = acc;
      }
    }
    wave_sync();
  }
}

}  // namespace

#endif  // MSPOSTERIOR_GROUPED_DEVICE_H
