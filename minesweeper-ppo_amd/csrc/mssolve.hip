// Avoidability analysis on device (include/mssolve.h): one wavefront per board.
//
// The board sits in LDS as row bitboards (row r at index r + 1, column c at bit c + 1, so a
// cell's 3x3 window is three shifts with no edge cases), lane r owns row r for the row-parallel
// steps and lane l owns cells l, l + 64, ... for the cell-parallel ones.
//   1 frontier      3x3 dilation of the revealed rows (DPP row shifts), minus revealed
//   2 components    min-label propagation through the constraint cells, LDS atomic min
//   3 closure       unit and strict-subset rules as 9-bit window logic, LDS atomic or
//   4 search        only if the closure proved nothing safe: per component, one query variable
//                   per lane, iterative depth-first search over 128-bit value strings
// Every loop has a bound fixed before it starts: label and closure rounds by the frontier size,
// the search by the node budget. A board the search cannot finish is reported undecided.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/mssolve.h"
#include "msenv_internal.h"
#include "mssolve_device.h"
#include "mssolve_host.h"

namespace {

constexpr int kWave = 64;
constexpr int kMaxCells = MS_AVOID_MAX_CELLS;
constexpr int kMaxVars = MS_AVOID_MAX_VARS;
constexpr uint32_t kNoLabel = 0xFFFFu;
constexpr uint16_t kNoCon = 0xFFFFu;

struct AvoidOut {
  uint8_t* status;
  uint8_t* avoidable;
  int32_t* n_safe;
  uint8_t* chosen_safe;
  int32_t* chosen_comp;
  int32_t* n_comp;
  int32_t* n_frontier;
  uint8_t* safe_mask;
  int32_t* max_nodes;
  int32_t* comp_size;
};

struct AvoidSrc {
  // a handle's packed planes (ms_avoid) ...
  const uint64_t* mine_words;
  const uint64_t* rev_words;
  const uint8_t* meta;
  int32_t meta_stride, flags_offset, NW;
  // ... or byte planes (ms_avoid_states)
  const uint8_t* rev_u8;
  const uint8_t* mine_u8;
  const uint8_t* first_click;
};

struct Lds {
  uint64_t rev[kWave + 2], mine[kWave + 2], fr[kWave + 2], safe[kWave + 2], fm[kWave + 2];
  uint32_t label[kMaxCells];  // component label of a frontier cell = its smallest cell index
  uint32_t count[kMaxCells];  // cells per label
  uint64_t cm_lo[kMaxCells], cm_hi[kMaxCells];  // a component's constraints over local variables
  int8_t ctarget[kMaxCells];
  uint8_t lvar[kMaxCells];             // cell -> local variable (search order) of the component in hand
  uint16_t vcell[kMaxVars];            // local variable -> cell
  uint16_t vcons[kMaxVars * 8];        // local variable -> its constraints, one slot per direction
};

__global__ __launch_bounds__(64) void k_avoid(AvoidSrc src, const int64_t* __restrict__ chosen_in,
                                              const uint8_t* __restrict__ live, int64_t n, int H, int W, int budget,
                                              AvoidOut o) {
  __shared__ Lds L;
  const int lane = lane_id();
  const int64_t env = blockIdx.x;
  if (env >= n) return;
  const int A = H * W;
  const bool handle = src.rev_words != nullptr;
  bool fc;
  if (handle)
    fc = (*(const uint32_t*)(src.meta + env * src.meta_stride + src.flags_offset) & 1u) != 0;
  else
    fc = src.first_click ? src.first_click[env] != 0 : true;
  const bool analysed = fc && (!live || live[env] != 0);
  const bool too_big = A > kMaxCells;

  uint8_t st = MS_AVOID_DECIDED, avoidable = 0, chosen_safe = 0;
  int32_t n_safe = 0, chosen_comp = 0, n_comp = 0, n_frontier = 0, max_nodes = 0;
  bool have_sets = false;  // L.safe / L.count hold this board's answer

  if (!analysed) {
    st = MS_AVOID_SKIPPED;
  } else if (too_big) {
    st = MS_AVOID_UNDECIDED;
  } else {
    int64_t ch64 = chosen_in[env] % A;
    if (ch64 < 0) ch64 += A;
    const int chosen = (int)ch64, chr = chosen / W, chc = chosen - chr * W;

    // ---- load: lane r builds row r
    uint64_t rev = 0, mine = 0;
    if (handle) {
      const int rpw = 64 / W;
      const int w = lane / rpw;
      const int wc = w < src.NW ? w : src.NW - 1;
      const int sh = (lane - w * rpw) * W;
      const uint64_t keep = lane < H ? (1ull << W) - 1ull : 0ull;
      rev = (src.rev_words[env * src.NW + wc] >> sh) & keep;
      mine = (src.mine_words[env * src.NW + wc] >> sh) & keep;
    } else if (lane < H) {
      const uint8_t* rp = src.rev_u8 + (env * H + lane) * W;
      const uint8_t* mp = src.mine_u8 + (env * H + lane) * W;
      for (int c = 0; c < W; ++c) {
        rev |= (uint64_t)(rp[c] != 0) << c;
        mine |= (uint64_t)(mp[c] != 0) << c;
      }
    }
    // ---- 1 frontier
    const uint64_t u = rev | wave_shr1(rev) | wave_shl1(rev);
    const uint64_t rowmask = lane < H ? (1ull << W) - 1ull : 0ull;
    const uint64_t fr = (u | (u << 1) | (u >> 1)) & ~rev & rowmask;
    L.rev[lane + 1] = rev << 1;
    L.mine[lane + 1] = mine << 1;
    L.fr[lane + 1] = fr << 1;
    L.safe[lane + 1] = 0;
    L.fm[lane + 1] = 0;
    if (lane == 0) {
      L.rev[0] = L.mine[0] = L.fr[0] = L.safe[0] = L.fm[0] = 0;
      L.rev[kWave + 1] = L.mine[kWave + 1] = L.fr[kWave + 1] = L.safe[kWave + 1] = L.fm[kWave + 1] = 0;
    }
    n_frontier = wave_sum(__popcll(fr));
    wave_sync();
    if (n_frontier == 0) {
      chosen_comp = cell_bit(L.rev, chr, chc) ? 0 : 1;
    } else {
      have_sets = true;
      // ---- 2 components
      for (int base = 0; base < A; base += kWave) {
        const int i = base + lane;
        if (i < A) {
          const int r = i / W, c = i - r * W;
          L.label[i] = cell_bit(L.fr, r, c) ? (uint32_t)i : kNoLabel;
          L.count[i] = 0;
        }
      }
      wave_sync();
      for (int round = 0; round <= n_frontier; ++round) {
        bool changed = false;
        for (int base = 0; base < A; base += kWave) {
          const int i = base + lane;
          if (i < A) {
            const int r = i / W, c = i - r * W;
            const uint32_t v = cell_bit(L.rev, r, c) && !cell_bit(L.mine, r, c) ? (win9(L.fr, r, c) & ~16u) : 0u;
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
        if (i < A && L.label[i] != kNoLabel) {
          atomicAdd(&L.count[L.label[i]], 1u);
          roots += L.label[i] == (uint32_t)i;
        }
      }
      n_comp = wave_sum(roots);
      wave_sync();
      if (cell_bit(L.fr, chr, chc)) chosen_comp = (int32_t)L.count[L.label[chosen]];

      // ---- 3 closure
      for (int round = 0; round <= n_frontier; ++round) {
        bool changed = false;
        for (int base = 0; base < A; base += kWave) {  // unit rule
          const int i = base + lane;
          if (i < A) {
            const int r = i / W, c = i - r * W;
            if (cell_bit(L.rev, r, c) && !cell_bit(L.mine, r, c)) {
              const uint32_t v = win9(L.fr, r, c) & ~16u, m = win9(L.fm, r, c);
              const uint32_t rem = v & ~win9(L.safe, r, c) & ~m;
              const int t = __popc(win9(L.mine, r, c) & ~16u) - __popc(v & m), nr = __popc(rem);
              if (rem && t == 0) {
                or9(L.safe, r, c, rem);
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
            if (cell_bit(L.rev, r, c) && !cell_bit(L.mine, r, c)) {
              const uint32_t va = win9(L.fr, r, c) & ~16u, ma = win9(L.fm, r, c);
              const uint32_t rema = va & ~win9(L.safe, r, c) & ~ma;
              const int ta = __popc(win9(L.mine, r, c) & ~16u) - __popc(va & ma);
              if (rema) {
#pragma unroll
                for (int dr = -2; dr <= 2; ++dr) {
#pragma unroll
                  for (int dc = -2; dc <= 2; ++dc) {
                    if (dr == 0 && dc == 0) continue;
                    const int rb = r + dr, cb = c + dc;
                    if (rb < 0 || rb >= H || cb < 0 || cb >= W) continue;
                    if (!cell_bit(L.rev, rb, cb) || cell_bit(L.mine, rb, cb)) continue;
                    bool lost;
                    const uint32_t ainb = shift9(rema, dr, dc, lost);
                    if (lost) continue;
                    const uint32_t vb = win9(L.fr, rb, cb) & ~16u, mb = win9(L.fm, rb, cb);
                    const uint32_t remb = vb & ~win9(L.safe, rb, cb) & ~mb;
                    const uint32_t diff = remb & ~ainb;
                    if ((ainb & ~remb) || !diff) continue;
                    const int tb = __popc(win9(L.mine, rb, cb) & ~16u) - __popc(vb & mb);
                    if (ta == tb) {
                      or9(L.safe, rb, cb, diff);
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
      n_safe = wave_sum(__popcll(L.safe[lane + 1]));

      // ---- 4 search, per component (roots in ascending cell order)
      if (n_safe == 0) {
        bool undecided = false;
        int nodes_max = 0;
        for (int rbase = 0; rbase < A; rbase += kWave) {
          const int ri = rbase + lane;
          uint64_t rootmask = ballot(ri < A && L.label[ri] == (uint32_t)ri);
          while (rootmask) {
            const uint32_t root = (uint32_t)(rbase + __builtin_ctzll(rootmask));
            rootmask &= rootmask - 1ull;
            // free cells of this component by degree (constraints per cell), 8 .. 0
            int cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int base = 0; base < A; base += kWave) {
              const int i = base + lane;
              int deg = -1;
              if (i < A && L.label[i] == root) {
                const int r = i / W, c = i - r * W;
                if (!cell_bit(L.fm, r, c)) deg = __popc(win9(L.rev, r, c) & ~win9(L.mine, r, c) & ~16u);
              }
#pragma unroll
              for (int d = 0; d < 9; ++d) cnt[d] += __popcll(ballot(deg == d));
            }
            int nv = 0;
#pragma unroll
            for (int d = 0; d < 9; ++d) nv += cnt[d];
            if (nv == 0) continue;
            if (nv > kMaxVars) {
              undecided = true;
              continue;
            }
            // search order: degree descending, then cell ascending
            int run[9];
            {
              int acc = 0;
#pragma unroll
              for (int d = 8; d >= 0; --d) {
                run[d] = acc;
                acc += cnt[d];
              }
            }
            for (int base = 0; base < A; base += kWave) {
              const int i = base + lane;
              int deg = -1;
              if (i < A && L.label[i] == root) {
                const int r = i / W, c = i - r * W;
                if (!cell_bit(L.fm, r, c)) deg = __popc(win9(L.rev, r, c) & ~win9(L.mine, r, c) & ~16u);
              }
              int rank = -1;
#pragma unroll
              for (int d = 0; d < 9; ++d) {
                const uint64_t b = ballot(deg == d);
                if (deg == d) rank = run[d] + __popcll(b & lanes_below(lane));
                run[d] += __popcll(b);
              }
              if (i < A) L.lvar[i] = rank >= 0 ? (uint8_t)rank : (uint8_t)0xFF;
              if (rank >= 0) {
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
                if (cell_bit(L.rev, r, c) && !cell_bit(L.mine, r, c)) {
                  const uint32_t v = win9(L.fr, r, c) & ~16u, m = win9(L.fm, r, c);
                  if (v && L.label[win_cell(i, W, __builtin_ctz(v))] == root) {
                    rem = v & ~m;
                    t = __popc(win9(L.mine, r, c) & ~16u) - __popc(v & m);
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
                L.cm_lo[ci] = mask.lo;
                L.cm_hi[ci] = mask.hi;
                L.ctarget[ci] = (int8_t)t;
              }
              nc += __popcll(b);
            }
            wave_sync();
            // queries: is "variable q is a mine" satisfiable? one q per lane
            for (int q0 = 0; q0 < nv; q0 += kWave) {
              const int q = q0 + lane;
              const Bits128 qbit = bit128(q < nv ? q : 0);
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
              // res: 0 searching, 1 satisfiable, 2 unsatisfiable (q is safe), 3 out of budget
              int res = q < nv ? 0 : 1;
              Bits128 val = qbit;
              int nodes = q < nv ? 1 : 0;
              if (res == 0 && !consistent(q, val, qbit)) res = 2;
              int d = q == 0 ? 1 : 0, x = 0;
              bool back = false;
              const int64_t iter_cap = 2 * (int64_t)budget + 2 * nv + 8;
              for (int64_t iter = 0; iter < iter_cap; ++iter) {
                if (!wave_any(res == 0)) break;
                if (res != 0) {
                  // this lane's query is answered; it idles until the wave's last one is
                } else if (!back) {
                  if (d >= nv) {
                    res = 1;
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
              if (res == 2) {
                const int cell = L.vcell[q];
                const int r = cell / W, c = cell - r * W;
                atomicOr((unsigned long long*)&L.safe[r + 1], 1ull << (c + 1));
              }
              undecided |= wave_any(res == 3);
              nodes_max = max(nodes_max, nodes);
            }
            wave_sync();
          }
        }
        max_nodes = wave_max(nodes_max);
        if (undecided) st = MS_AVOID_UNDECIDED;
        n_safe = wave_sum(__popcll(L.safe[lane + 1]));
      }
      if (st == MS_AVOID_UNDECIDED) {
        n_safe = 0;
      } else {
        avoidable = n_safe > 0;
        chosen_safe = cell_bit(L.safe, chr, chc);
      }
    }
  }

  if (lane == 0) {
    if (o.status) o.status[env] = st;
    if (o.avoidable) o.avoidable[env] = avoidable;
    if (o.n_safe) o.n_safe[env] = n_safe;
    if (o.chosen_safe) o.chosen_safe[env] = chosen_safe;
    if (o.chosen_comp) o.chosen_comp[env] = chosen_comp;
    if (o.n_comp) o.n_comp[env] = n_comp;
    if (o.n_frontier) o.n_frontier[env] = n_frontier;
    if (o.max_nodes) o.max_nodes[env] = max_nodes;
  }
  const bool masks = have_sets && st == MS_AVOID_DECIDED;
  for (int base = 0; base < A; base += kWave) {
    const int i = base + lane;
    if (i >= A) break;
    const int r = i / W, c = i - r * W;
    if (o.safe_mask) o.safe_mask[env * A + i] = masks ? (uint8_t)cell_bit(L.safe, r, c) : (uint8_t)0;
    if (o.comp_size)
      o.comp_size[env * A + i] = (have_sets && L.label[i] != kNoLabel) ? (int32_t)L.count[L.label[i]] : 0;
  }
}

int launch(const AvoidSrc& src, const int64_t* chosen, const uint8_t* live, int64_t n, int H, int W, int budget,
           const AvoidOut& o, void* stream, const char* who) {
  hipLaunchKernelGGL(k_avoid, dim3((unsigned)n), dim3(kWave), 0, (hipStream_t)stream, src, chosen, live, n, H, W,
                     budget, o);
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return MS_OK;
  char msg[256];
  snprintf(msg, sizeof msg, "%s launch: %s", who, hipGetErrorString(e));
  return ms_internal_fail(MS_EHIP, msg);
}

bool budget_ok(int32_t b) { return b >= 1 && b <= (1 << 30); }

}  // namespace

extern "C" {

int ms_avoid_set_budget(ms_handle* h, int32_t nodes) {
  if (!h) return ms_internal_fail(MS_EINVAL, "ms_avoid_set_budget: null handle");
  if (!budget_ok(nodes)) return ms_internal_fail(MS_EINVAL, "ms_avoid_set_budget: need 1 <= nodes <= 2^30");
  ms_board_view v;
  ms_internal_board_view(h, &v);
  *v.avoid_budget = nodes;
  return MS_OK;
}

int ms_avoid(ms_handle* h, const int64_t* chosen, const uint8_t* live, uint8_t* status, uint8_t* avoidable,
             int32_t* n_safe, uint8_t* chosen_safe, int32_t* chosen_comp, int32_t* n_comp, int32_t* n_frontier,
             uint8_t* safe_mask, int32_t* max_nodes, int32_t* comp_size, void* stream) {
  if (!h) return ms_internal_fail(MS_EINVAL, "ms_avoid: null handle");
  if (!chosen) return ms_internal_fail(MS_EINVAL, "ms_avoid: null chosen");
  ms_board_view v;
  ms_internal_board_view(h, &v);
  AvoidSrc src = {};
  src.mine_words = v.mine_words;
  src.rev_words = v.rev_words;
  src.meta = v.meta;
  src.meta_stride = v.meta_stride;
  src.flags_offset = v.flags_offset;
  src.NW = v.NW;
  const AvoidOut o = {status, avoidable, n_safe, chosen_safe, chosen_comp, n_comp, n_frontier, safe_mask, max_nodes,
                      comp_size};
  const int budget = *v.avoid_budget ? *v.avoid_budget : MS_AVOID_DEFAULT_BUDGET;
  return launch(src, chosen, live, v.n, v.H, v.W, budget, o, stream, "ms_avoid");
}

int ms_avoid_states(const uint8_t* revealed, const uint8_t* mine, const uint8_t* first_click, const int64_t* chosen,
                    const uint8_t* live, int64_t n, int32_t H, int32_t W, int32_t budget, uint8_t* status,
                    uint8_t* avoidable, int32_t* n_safe, uint8_t* chosen_safe, int32_t* chosen_comp, int32_t* n_comp,
                    int32_t* n_frontier, uint8_t* safe_mask, int32_t* max_nodes, int32_t* comp_size, void* stream) {
  if (!revealed || !mine || !chosen) return ms_internal_fail(MS_EINVAL, "ms_avoid_states: null revealed, mine or chosen");
  if (n <= 0 || n > 0x7fffffffll) return ms_internal_fail(MS_EINVAL, "ms_avoid_states: need 1 <= n < 2^31");
  if (H < 1 || H > 64 || W < 1 || W > 62) return ms_internal_fail(MS_EINVAL, "ms_avoid_states: need 1<=H<=64, 1<=W<=62");
  if (!budget_ok(budget)) return ms_internal_fail(MS_EINVAL, "ms_avoid_states: need 1 <= budget <= 2^30");
  AvoidSrc src = {};
  src.rev_u8 = revealed;
  src.mine_u8 = mine;
  src.first_click = first_click;
  const AvoidOut o = {status, avoidable, n_safe, chosen_safe, chosen_comp, n_comp, n_frontier, safe_mask, max_nodes,
                      comp_size};
  return launch(src, chosen, live, n, H, W, budget, o, stream, "ms_avoid_states");
}

int ms_avoid_host(const uint8_t* revealed, const uint8_t* mine, const uint8_t* first_click, const int64_t* chosen,
                  const uint8_t* live, int64_t n, int32_t H, int32_t W, uint8_t* status, uint8_t* avoidable,
                  int32_t* n_safe, uint8_t* chosen_safe, int32_t* chosen_comp, int32_t* n_comp, int32_t* n_frontier,
                  uint8_t* safe_mask, int32_t* max_nodes, int32_t* comp_size) {
  if (!revealed || !mine || !chosen) return ms_internal_fail(MS_EINVAL, "ms_avoid_host: null revealed, mine or chosen");
  if (n <= 0) return ms_internal_fail(MS_EINVAL, "ms_avoid_host: need n >= 1");
  if (H < 1 || W < 1 || (int64_t)H * W > (1 << 20)) return ms_internal_fail(MS_EINVAL, "ms_avoid_host: need H, W >= 1 and H*W <= 2^20");
  const int64_t A = (int64_t)H * W;
  for (int64_t e = 0; e < n; ++e) {
    uint8_t* sm = safe_mask ? safe_mask + e * A : nullptr;
    int32_t* cs = comp_size ? comp_size + e * A : nullptr;
    mssolve::Result R;
    if ((first_click && !first_click[e]) || (live && !live[e])) {
      if (sm) std::fill(sm, sm + A, (uint8_t)0);
      if (cs) std::fill(cs, cs + A, 0);
    } else {
      R = mssolve::analyze(revealed + e * A, mine + e * A, H, W, chosen[e], sm, cs);
    }
    if (status) status[e] = R.status;
    if (avoidable) avoidable[e] = R.avoidable;
    if (n_safe) n_safe[e] = R.n_safe;
    if (chosen_safe) chosen_safe[e] = R.chosen_safe;
    if (chosen_comp) chosen_comp[e] = R.chosen_comp;
    if (n_comp) n_comp[e] = R.n_comp;
    if (n_frontier) n_frontier[e] = R.n_frontier;
    if (max_nodes) max_nodes[e] = R.max_nodes;
  }
  return MS_OK;
}

}  // extern "C"
