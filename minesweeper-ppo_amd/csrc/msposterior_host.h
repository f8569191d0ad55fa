// Exact mine-probability posterior (include/msposterior.h, and with grouped counting
// include/msposterior_grouped.h) in plain C++: no HIP, no size cap,
// an optional node budget. It is the exact fallback for boards the device kernel leaves
// undecided (ms_posterior_host) and, being ordinary host code, can be compiled into a
// stand-alone program under sanitizers (tools/msposterior_hostcheck.cpp).
//
// It is written cell by cell with explicit index lists, on purpose unlike the kernel's bitboard
// form (csrc/msposterior.hip), so that the two check each other. Only the search's state machine
// is the same, step for step, so that both count the same nodes and the same solutions. The
// grouped counting is unlike the kernel's in the same way: a map from constraint set to group and
// running sums per constraint here, byte strings and a walk over group lists there.
#ifndef MSPOSTERIOR_HOST_H
#define MSPOSTERIOR_HOST_H

#include <stdint.h>

#include <algorithm>
#include <map>
#include <type_traits>
#include <vector>

namespace msposterior {

enum { kSkipped = 0, kDecided = 1, kUndecided = 2, kInconsistent = 3 };

struct Result {
  int status = kSkipped;  // kInconsistent: no layout reproduces the numbers (Z = 0)
  double configs = 0.0;
  int32_t max_nodes = 0;
};

// Counts the 0/1 assignments of the nv variables (numbered in search order) that give every
// constraint c exactly target[c] mines among its variables, with variable q a mine (q < 0: no
// such condition): hist[k] += 1 per solution with k mines. Depth-first, value 0 before 1,
// pruning a constraint as soon as its mines exceed the target or mines plus unassigned fall
// short of it. *nodes = attempted assignments (q's included). budget 0 = unbounded; returns
// false if the query was stopped at `budget` nodes.
inline bool count_solutions(int nv, const std::vector<std::vector<int>>& vcons, const std::vector<int>& target,
                            const std::vector<int>& csize, int q, int64_t budget, std::vector<uint64_t>& hist,
                            int64_t* nodes) {
  const size_t nc = target.size();
  std::vector<int> mines(nc, 0), unknown(csize);
  std::vector<int8_t> val((size_t)nv, -1);
  int total = 0;
  auto assign = [&](int v, int x) {
    bool ok = true;
    for (int c : vcons[(size_t)v]) {
      mines[(size_t)c] += x;
      unknown[(size_t)c] -= 1;
      if (mines[(size_t)c] > target[(size_t)c] || mines[(size_t)c] + unknown[(size_t)c] < target[(size_t)c]) ok = false;
    }
    if (ok) {
      val[(size_t)v] = (int8_t)x;
      total += x;
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
    total -= x;
    val[(size_t)v] = -1;
  };
  *nodes = 0;
  if (q >= 0) {
    *nodes = 1;
    if (!assign(q, 1)) return true;
  }
  int d = q == 0 ? 1 : 0, x = 0;
  bool back = false;
  for (;;) {
    if (!back) {
      if (d >= nv) {
        hist[(size_t)total] += 1;  // a leaf: count it and go on
        back = true;
      } else if (budget > 0 && *nodes >= budget) {
        return false;
      } else {
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
      }
    } else {
      d -= 1;
      if (d == q) d -= 1;
      if (d < 0) return true;
      const bool was1 = val[(size_t)d] == 1;
      unassign(d);
      if (!was1) {
        x = 1;
        back = false;
      }
    }
  }
}

// The grouped counting of include/msposterior_grouped.h: the ng groups (numbered in search order)
// are variables with values 0 .. mult[g], gcons[g] lists a group's constraints. With q >= 0 the
// smallest cell of group q is a mine: it is fixed before the search, lowers the targets of q's
// constraints by one and leaves q with one cell fewer (q is passed over when none is left).
// Depth-first, value 0 first; a constraint is pruned as soon as its assigned sum exceeds the
// target or the assigned sum plus the multiplicities still open falls short of it. A leaf with
// values v adds prod_g C(mult[g], v[g]), multiplied in ascending g, to hist[sum v (+ 1 for q)].
// *nodes = attempted values (the fixed cell of q counts as one). budget 0 = unbounded; returns
// false if the query was stopped at `budget` nodes.
inline double small_binomial(int n, int v) {  // C(n, v) for 0 <= v <= n <= 8
  double c = 1.0;
  for (int i = 0; i < v; ++i) c = c * (double)(n - i) / (double)(i + 1);
  return c;
}

inline bool count_grouped(const std::vector<int>& mult, const std::vector<std::vector<int>>& gcons,
                          const std::vector<int>& target, const std::vector<int>& csize, int q, int64_t budget,
                          std::vector<double>& hist, int64_t* nodes) {
  const int ng = (int)mult.size();
  const size_t nc = target.size();
  std::vector<int> left(mult), goal(target), mines(nc, 0), open(csize);
  std::vector<int> val((size_t)ng, 0);
  int total = 0;
  auto fits = [&](int g) {
    for (int c : gcons[(size_t)g])
      if (mines[(size_t)c] > goal[(size_t)c] || mines[(size_t)c] + open[(size_t)c] < goal[(size_t)c]) return false;
    return true;
  };
  auto assign = [&](int g, int x) {
    for (int c : gcons[(size_t)g]) {
      mines[(size_t)c] += x;
      open[(size_t)c] -= left[(size_t)g];
    }
    if (fits(g)) {
      val[(size_t)g] = x;
      total += x;
      return true;
    }
    for (int c : gcons[(size_t)g]) {
      mines[(size_t)c] -= x;
      open[(size_t)c] += left[(size_t)g];
    }
    return false;
  };
  auto unassign = [&](int g) {
    for (int c : gcons[(size_t)g]) {
      mines[(size_t)c] -= val[(size_t)g];
      open[(size_t)c] += left[(size_t)g];
    }
    total -= val[(size_t)g];
    val[(size_t)g] = 0;
  };
  *nodes = 0;
  int skip = -1;
  if (q >= 0) {
    *nodes = 1;
    total = 1;
    left[(size_t)q] -= 1;
    if (left[(size_t)q] == 0) skip = q;
    for (int c : gcons[(size_t)q]) {
      goal[(size_t)c] -= 1;
      open[(size_t)c] -= 1;
    }
    if (!fits(q)) return true;
  }
  int d = skip == 0 ? 1 : 0, x = 0;
  bool back = false;
  for (;;) {
    if (!back) {
      if (d >= ng) {  // a leaf: weigh it and go on
        double w = 1.0;
        for (int g = 0; g < ng; ++g) w *= small_binomial(left[(size_t)g], val[(size_t)g]);
        hist[(size_t)total] += w;
        back = true;
      } else if (budget > 0 && *nodes >= budget) {
        return false;
      } else {
        ++*nodes;
        if (assign(d, x)) {
          d += 1;
          if (d == skip) d += 1;
          x = 0;
        } else if (x < left[(size_t)d]) {
          x += 1;
        } else {
          back = true;
        }
      }
    } else {
      d -= 1;
      if (d == skip) d -= 1;
      if (d < 0) return true;
      const int was = val[(size_t)d];
      unassign(d);
      if (was < left[(size_t)d]) {
        x = was + 1;
        back = false;
      }
    }
  }
}

// row[r] = C(n, r) for 0 <= r <= rmax by the multiplicative recurrence (exact while the values
// stay below 2^53), 0 for r > n
inline void binomial_row(int n, int rmax, std::vector<double>& row) {
  row.assign((size_t)rmax + 1, 0.0);
  if (n < 0) return;
  row[0] = 1.0;
  for (int r = 0; r < rmax && r < n; ++r) row[(size_t)r + 1] = row[(size_t)r] * (double)(n - r) / (double)(r + 1);
}

// V[m] <- sum_s N[s] V[m + s]: folds one component's counts into a binomial tail
template <typename Count>
inline void absorb(std::vector<double>& V, const std::vector<Count>& N) {
  const size_t len = V.size();
  for (size_t m = 0; m < len; ++m) {
    double acc = 0.0;
    for (size_t s = 0; s < N.size() && m + s < len; ++s) acc += (double)N[s] * V[m + s];
    V[m] = acc;
  }
}

// revealed / number: H*W bytes (number is read at revealed cells only). prob: H*W entries or
// null. budget: nodes per query, 0 = unbounded. Count = uint64_t: the enumerating search
// (count_solutions); Count = double: the grouped one (count_grouped). Everything around the
// per-component counting is the same code, so wherever both decide their counts are the same
// integers, combined in the same order.
template <typename Count>
inline Result analyze_impl(const uint8_t* revealed, const uint8_t* number, int H, int W, int M, int64_t budget,
                           double* prob) {
  constexpr bool kGrouped = std::is_same<Count, double>::value;
  const int A = H * W;
  Result R;
  if (prob) std::fill(prob, prob + A, 0.0);
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
  int n_revealed = 0, n_frontier = 0;
  std::vector<uint8_t> frontier((size_t)A, 0);
  for (int i = 0; i < A; ++i) {
    if (revealed[i]) {
      n_revealed += 1;
      continue;
    }
    const int k = nbrs(i, nb);
    for (int j = 0; j < k; ++j)
      if (revealed[nb[j]]) frontier[(size_t)i] = 1;
    n_frontier += frontier[(size_t)i];
  }
  if (n_revealed == 0) return R;  // nothing to condition on: skipped
  R.status = kInconsistent;

  struct Con {
    int cell, target;
    std::vector<int> vars;
  };
  std::vector<Con> cons;
  std::vector<int> con_of((size_t)A, -1);
  for (int i = 0; i < A; ++i) {
    if (!revealed[i]) continue;
    Con c;
    c.cell = i;
    c.target = number[i];
    const int k = nbrs(i, nb);
    for (int j = 0; j < k; ++j)
      if (frontier[(size_t)nb[j]]) c.vars.push_back(nb[j]);
    if (c.vars.empty()) {
      if (c.target != 0) return R;
      continue;
    }
    con_of[(size_t)i] = (int)cons.size();
    cons.push_back(c);
  }

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
        if (k == 0 || (t != 0 && t != k)) continue;
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
  // what the closure left must still be satisfiable constraint by constraint
  int closure_mines = 0;
  for (int i = 0; i < A; ++i) closure_mines += state[(size_t)i] == 1;
  for (const Con& c : cons) {
    int rem[8], t;
    const int k = remaining(c, rem, &t);
    if (t < 0 || t > k) return R;
  }
  const int Rm = M - closure_mines;                       // mines left for free and interior cells
  const int U = A - n_revealed - n_frontier;              // interior cells
  if (Rm < 0) return R;

  // components of the reduced system: free cells joined through each constraint's free cells
  std::vector<int> parent((size_t)A);
  for (int i = 0; i < A; ++i) parent[(size_t)i] = i;
  auto find = [&](int x) {
    while (parent[(size_t)x] != x) x = parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
    return x;
  };
  for (const Con& c : cons) {
    int rem[8], t;
    const int k = remaining(c, rem, &t);
    for (int j = 1; j < k; ++j) {
      const int a = find(rem[0]), b = find(rem[j]);
      if (a != b) parent[(size_t)std::max(a, b)] = std::min(a, b);
    }
  }

  // counts, per component in ascending order of its smallest cell
  struct Comp {
    std::vector<int> vars;                    // cells in search order (ascending)
    std::vector<Count> N;                     // N[k]
    std::vector<std::vector<Count>> Nv;       // Nv[v][k]
  };
  std::vector<Comp> comps;
  std::vector<int> local((size_t)A, -1);
  int64_t max_nodes = 0;
  bool stopped = false;
  for (int root = 0; root < A && !stopped; ++root) {
    if (!frontier[(size_t)root] || state[(size_t)root] >= 0 || find(root) != root) continue;
    Comp C;
    for (int i = root; i < A; ++i)
      if (frontier[(size_t)i] && state[(size_t)i] < 0 && find(i) == root) C.vars.push_back(i);
    const int nv = (int)C.vars.size();
    for (int k = 0; k < nv; ++k) local[(size_t)C.vars[(size_t)k]] = k;
    std::vector<std::vector<int>> vcons((size_t)nv);
    std::vector<int> target, csize;
    for (const Con& c : cons) {
      int rem[8], t;
      const int k = remaining(c, rem, &t);
      if (k == 0 || find(rem[0]) != root) continue;
      for (int j = 0; j < k; ++j) vcons[(size_t)local[(size_t)rem[j]]].push_back((int)target.size());
      target.push_back(t);
      csize.push_back(k);
    }
    C.N.assign((size_t)nv + 1, 0);
    C.Nv.assign((size_t)nv, std::vector<Count>((size_t)nv + 1, 0));
    if constexpr (kGrouped) {
      // groups: cells with the same constraint set, numbered by their smallest cell
      std::map<std::vector<int>, int> group_of;
      std::vector<int> mult, vgroup((size_t)nv);
      std::vector<std::vector<int>> gcons;
      for (int v = 0; v < nv; ++v) {
        const auto at = group_of.emplace(vcons[(size_t)v], (int)mult.size());  // vcons[v] is ascending
        if (at.second) {
          mult.push_back(0);
          gcons.push_back(vcons[(size_t)v]);
        }
        vgroup[(size_t)v] = at.first->second;
        mult[(size_t)at.first->second] += 1;
      }
      const int ng = (int)mult.size();
      std::vector<std::vector<Count>> Ng((size_t)ng, std::vector<Count>((size_t)nv + 1, 0));
      for (int q = -1; q < ng && !stopped; ++q) {
        int64_t nodes = 0;
        if (!count_grouped(mult, gcons, target, csize, q, budget, q < 0 ? C.N : Ng[(size_t)q], &nodes)) stopped = true;
        max_nodes = std::max(max_nodes, nodes);
      }
      for (int v = 0; v < nv; ++v) C.Nv[(size_t)v] = Ng[(size_t)vgroup[(size_t)v]];  // the cells of a group are symmetric
    } else {
      for (int q = -1; q < nv; ++q) {
        int64_t nodes = 0;
        if (!count_solutions(nv, vcons, target, csize, q, budget, q < 0 ? C.N : C.Nv[(size_t)q], &nodes)) stopped = true;
        max_nodes = std::max(max_nodes, nodes);
      }
    }
    comps.push_back(std::move(C));
  }
  R.max_nodes = (int32_t)std::min<int64_t>(max_nodes, INT32_MAX);
  if (stopped) {
    R.status = kUndecided;
    return R;
  }

  // combine: B[m] = C(U, Rm - m); folding every component but j into B gives W_j[k]
  std::vector<double> row;
  binomial_row(U, Rm, row);
  auto tail = [&](const std::vector<double>& rw, int top) {  // V[m] = rw[top - m], m = 0 .. top
    std::vector<double> V((size_t)std::max(top, -1) + 1);
    for (int m = 0; m <= top; ++m) V[(size_t)m] = rw[(size_t)(top - m)];
    return V;
  };
  std::vector<double> V = tail(row, Rm);
  for (const Comp& C : comps) absorb(V, C.N);
  const double Z = V[0];
  if (!(Z > 0.0)) {
    R.max_nodes = 0;
    return R;
  }
  R.status = kDecided;
  R.configs = Z;
  if (!prob) return R;
  for (int i = 0; i < A; ++i)
    if (state[(size_t)i] == 1) prob[i] = 1.0;
  for (size_t j = 0; j < comps.size(); ++j) {
    std::vector<double> Wj = tail(row, Rm);
    for (size_t i = 0; i < comps.size(); ++i)
      if (i != j) absorb(Wj, comps[i].N);
    const Comp& C = comps[j];
    for (size_t v = 0; v < C.vars.size(); ++v) {
      double acc = 0.0;
      for (size_t k = 0; k < C.Nv[v].size() && k < Wj.size(); ++k) acc += (double)C.Nv[v][k] * Wj[k];
      prob[C.vars[v]] = std::min(acc / Z, 1.0);  // a sure mine may round to 1 + 1 ulp
    }
  }
  if (U > 0 && Rm > 0) {
    binomial_row(U - 1, Rm - 1, row);
    std::vector<double> Vi = tail(row, Rm - 1);
    for (const Comp& C : comps) absorb(Vi, C.N);
    const double pi = std::min(Vi[0] / Z, 1.0);
    for (int i = 0; i < A; ++i)
      if (!revealed[i] && !frontier[(size_t)i]) prob[i] = pi;
  }
  return R;
}

inline Result analyze(const uint8_t* revealed, const uint8_t* number, int H, int W, int M, int64_t budget,
                      double* prob) {
  return analyze_impl<uint64_t>(revealed, number, H, W, M, budget, prob);
}

// include/msposterior_grouped.h
inline Result analyze_grouped(const uint8_t* revealed, const uint8_t* number, int H, int W, int M, int64_t budget,
                              double* prob) {
  return analyze_impl<double>(revealed, number, H, W, M, budget, prob);
}

}  // namespace msposterior

#endif  // MSPOSTERIOR_HOST_H
