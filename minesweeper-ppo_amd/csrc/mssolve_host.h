// Avoidability analysis (include/mssolve.h) in plain C++: no HIP, no budget, no size cap.
// It is the exact fallback for boards the device kernel leaves undecided (ms_avoid_host) and,
// being ordinary host code, can be compiled into a stand-alone program under sanitizers.
//
// It is written cell by cell with explicit index lists, on purpose unlike the kernel's bitboard
// form (csrc/mssolve.hip), so that the two check each other. Only the search's state machine
// is the same, step for step, so that both count the same nodes.
#ifndef MSSOLVE_HOST_H
#define MSSOLVE_HOST_H

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace mssolve {

struct Result {
  uint8_t status = 0, avoidable = 0, chosen_safe = 0;
  int32_t n_safe = 0, chosen_comp = 0, n_comp = 0, n_frontier = 0, max_nodes = 0;
};

// Is there a 0/1 assignment of the nv variables (numbered in search order) that gives every
// constraint c exactly target[c] mines among cvars[c], with variable q a mine? Depth-first,
// value 0 before 1, pruning a constraint as soon as its mines exceed the target or mines plus
// unassigned fall short of it. *nodes = attempted assignments (q's included).
inline bool feasible_with_mine(int nv, const std::vector<std::vector<int>>& vcons, const std::vector<int>& target,
                               const std::vector<int>& csize, int q, int64_t* nodes) {
  const size_t nc = target.size();
  std::vector<int> mines(nc, 0), unknown(csize);
  std::vector<int8_t> val((size_t)nv, -1);
  auto assign = [&](int v, int x) {
    bool ok = true;
    for (int c : vcons[(size_t)v]) {
      mines[(size_t)c] += x;
      unknown[(size_t)c] -= 1;
      if (mines[(size_t)c] > target[(size_t)c] || mines[(size_t)c] + unknown[(size_t)c] < target[(size_t)c]) ok = false;
    }
    if (ok) {
      val[(size_t)v] = (int8_t)x;
      return true;
    }
    for (int c : vcons[(size_t)v]) {
      mines[(size_t)c] -= x;
      unknown[(size_t)c] += 1;
    }
    return false;
  };
  auto unassign = [&](int v) {
    const int x = val[(size_t)v];
    for (int c : vcons[(size_t)v]) {
      mines[(size_t)c] -= x;
      unknown[(size_t)c] += 1;
    }
    val[(size_t)v] = -1;
  };
  *nodes = 1;
  if (!assign(q, 1)) return false;
  int d = q == 0 ? 1 : 0, x = 0;
  bool back = false;
  for (;;) {
    if (!back) {
      if (d >= nv) return true;
      ++*nodes;
      if (assign(d, x)) {
        d += 1;
        if (d == q) d += 1;
        x = 0;
      } else if (x == 0) {
        x = 1;
      } else {
        back = true;
      }
    } else {
      d -= 1;
      if (d == q) d -= 1;
      if (d < 0) return false;
      const bool was1 = val[(size_t)d] == 1;
      unassign(d);
      if (!was1) {
        x = 1;
        back = false;
      }
    }
  }
}

// revealed / mine: H*W bytes (nonzero = set). safe_mask / comp_size: H*W entries or null.
inline Result analyze(const uint8_t* revealed, const uint8_t* mine, int H, int W, int64_t chosen_raw,
                      uint8_t* safe_mask, int32_t* comp_size) {
  const int A = H * W;
  Result R;
  R.status = 1;
  if (safe_mask) std::fill(safe_mask, safe_mask + A, (uint8_t)0);
  if (comp_size) std::fill(comp_size, comp_size + A, 0);
  const int chosen = (int)(((chosen_raw % A) + A) % A);
  auto nbrs = [&](int cell, int* out) {  // in-board 8-neighbours
    const int r = cell / W, c = cell % W;
    int k = 0;
    for (int dr = -1; dr <= 1; ++dr)
      for (int dc = -1; dc <= 1; ++dc) {
        if (!dr && !dc) continue;
        const int rr = r + dr, cc = c + dc;
        if (rr >= 0 && rr < H && cc >= 0 && cc < W) out[k++] = rr * W + cc;
      }
    return k;
  };
  int nb[8];
  std::vector<uint8_t> frontier((size_t)A, 0);
  for (int i = 0; i < A; ++i) {
    if (revealed[i]) continue;
    const int k = nbrs(i, nb);
    for (int j = 0; j < k; ++j)
      if (revealed[nb[j]]) frontier[(size_t)i] = 1;
    R.n_frontier += frontier[(size_t)i];
  }
  if (R.n_frontier == 0) {
    R.chosen_comp = revealed[chosen] ? 0 : 1;
    return R;
  }

  struct Con {
    int cell, target;
    std::vector<int> vars;
  };
  std::vector<Con> cons;
  std::vector<int> con_of((size_t)A, -1);
  for (int i = 0; i < A; ++i) {
    if (!revealed[i] || mine[i]) continue;
    Con c;
    c.cell = i;
    c.target = 0;
    const int k = nbrs(i, nb);
    for (int j = 0; j < k; ++j) {
      c.target += mine[nb[j]] ? 1 : 0;
      if (frontier[(size_t)nb[j]]) c.vars.push_back(nb[j]);
    }
    if (c.vars.empty()) continue;
    con_of[(size_t)i] = (int)cons.size();
    cons.push_back(c);
  }

  // components: union-find over frontier cells, joined through each constraint
  std::vector<int> parent((size_t)A);
  for (int i = 0; i < A; ++i) parent[(size_t)i] = i;
  auto find = [&](int x) {
    while (parent[(size_t)x] != x) x = parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
    return x;
  };
  for (const Con& c : cons)
    for (size_t j = 1; j < c.vars.size(); ++j) {
      const int a = find(c.vars[0]), b = find(c.vars[j]);
      if (a != b) parent[(size_t)std::max(a, b)] = std::min(a, b);
    }
  std::vector<int> size((size_t)A, 0);
  for (int i = 0; i < A; ++i)
    if (frontier[(size_t)i]) size[(size_t)find(i)] += 1;
  for (int i = 0; i < A; ++i) {
    if (!frontier[(size_t)i]) continue;
    if (find(i) == i) R.n_comp += 1;
    if (comp_size) comp_size[i] = size[(size_t)find(i)];
  }
  if (frontier[(size_t)chosen]) R.chosen_comp = size[(size_t)find(chosen)];

  // closure of the unit and strict-subset rules; state: -1 unknown, 0 safe, 1 mine
  std::vector<int8_t> state((size_t)A, -1);
  auto remaining = [&](const Con& c, int* rem, int* t) {
    int k = 0;
    *t = c.target;
    for (int v : c.vars) {
      if (state[(size_t)v] < 0)
        rem[k++] = v;
      else if (state[(size_t)v] == 1)
        *t -= 1;
    }
    return k;
  };
  for (;;) {
    bool changed = false;
    for (bool again = true; again;) {  // unit rule to its own fixpoint first
      again = false;
      for (const Con& c : cons) {
        int rem[8], t;
        const int k = remaining(c, rem, &t);
        if (k == 0 || t < 0 || t > k || (t != 0 && t != k)) continue;
        for (int j = 0; j < k; ++j) state[(size_t)rem[j]] = t == 0 ? 0 : 1;
        again = changed = true;
      }
    }
    // one pass of the strict-subset rule over every ordered pair whose windows can overlap
    std::vector<std::pair<int, int8_t>> found;
    for (const Con& a : cons) {
      int ra[8], ta;
      const int ka = remaining(a, ra, &ta);
      if (ka == 0) continue;
      const int r = a.cell / W, c = a.cell % W;
      for (int dr = -2; dr <= 2; ++dr)
        for (int dc = -2; dc <= 2; ++dc) {
          const int rr = r + dr, cc = c + dc;
          if ((!dr && !dc) || rr < 0 || rr >= H || cc < 0 || cc >= W) continue;
          const int bi = con_of[(size_t)(rr * W + cc)];
          if (bi < 0) continue;
          int rb[8], tb;
          const int kb = remaining(cons[(size_t)bi], rb, &tb);
          if (kb <= ka) continue;  // a strict subset is smaller
          bool sub = true;
          for (int j = 0; j < ka && sub; ++j) sub = std::find(rb, rb + kb, ra[j]) != rb + kb;
          if (!sub) continue;
          int8_t v;
          if (ta == tb)
            v = 0;
          else if (tb - ta == kb - ka)
            v = 1;
          else
            continue;
          for (int j = 0; j < kb; ++j)
            if (std::find(ra, ra + ka, rb[j]) == ra + ka) found.push_back({rb[j], v});
        }
    }
    for (const auto& f : found)
      if (state[(size_t)f.first] < 0) {
        state[(size_t)f.first] = f.second;
        changed = true;
      }
    if (!changed) break;
  }
  auto finish = [&]() {
    for (int i = 0; i < A; ++i)
      if (state[(size_t)i] == 0) {
        R.n_safe += 1;
        if (safe_mask) safe_mask[i] = 1;
      }
    R.avoidable = R.n_safe > 0;
    R.chosen_safe = state[(size_t)chosen] == 0;
    return R;
  };
  for (int i = 0; i < A; ++i)
    if (state[(size_t)i] == 0) return finish();  // the closure proved a safe cell: no search

  // exact stage, per component over its free cells and reduced constraints
  std::vector<int> degree((size_t)A, 0), local((size_t)A, -1);
  for (const Con& c : cons)
    for (int v : c.vars)
      if (state[(size_t)v] < 0) degree[(size_t)v] += 1;
  int64_t max_nodes = 0;
  for (int root = 0; root < A; ++root) {
    if (!frontier[(size_t)root] || find(root) != root) continue;
    std::vector<int> vars;
    for (int i = root; i < A; ++i)
      if (frontier[(size_t)i] && state[(size_t)i] < 0 && find(i) == root) vars.push_back(i);
    if (vars.empty()) continue;
    // search order: most constrained first, ties by cell index
    std::stable_sort(vars.begin(), vars.end(), [&](int a, int b) { return degree[(size_t)a] > degree[(size_t)b]; });
    const int nv = (int)vars.size();
    for (int k = 0; k < nv; ++k) local[(size_t)vars[(size_t)k]] = k;
    std::vector<std::vector<int>> vcons((size_t)nv);
    std::vector<int> target, csize;
    for (const Con& c : cons) {
      if (find(c.vars[0]) != root) continue;
      int rem[8], t;
      const int k = remaining(c, rem, &t);
      if (k == 0) continue;
      for (int j = 0; j < k; ++j) vcons[(size_t)local[(size_t)rem[j]]].push_back((int)target.size());
      target.push_back(t);
      csize.push_back(k);
    }
    for (int q = 0; q < nv; ++q) {
      int64_t nodes = 0;
      if (!feasible_with_mine(nv, vcons, target, csize, q, &nodes)) state[(size_t)vars[(size_t)q]] = 0;
      max_nodes = std::max(max_nodes, nodes);
    }
  }
  R.max_nodes = (int32_t)std::min<int64_t>(max_nodes, INT32_MAX);
  return finish();
}

}  // namespace mssolve

#endif  // MSSOLVE_HOST_H
