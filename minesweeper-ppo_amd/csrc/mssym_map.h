// The cell map of the board symmetries (include/mssym.h), in one place: every kernel of
// mssym.hip, the host entry ms_sym_cell_map_host and tools/mssym_hostcheck.cpp use these.
// Plain C++ where no HIP compiler is at work, so it builds under host sanitizers.
#ifndef MSSYM_MAP_H
#define MSSYM_MAP_H

#if defined(__HIPCC__)
#define MSSYM_HD __host__ __device__
#else
#define MSSYM_HD
#endif

namespace mssym {

// 0..3 on any board, 4..7 (with the transpose) on square boards only
MSSYM_HD inline bool valid(int H, int W, unsigned g) { return g < 4u || (g < 8u && H == W); }

// T_{inverse(g)} undoes T_g: with the transpose, the two reversals trade places
MSSYM_HD inline unsigned inverse(unsigned g) { return g < 4u ? g : (4u | ((g & 1u) << 1) | ((g >> 1) & 1u)); }

// The source cell of output cell i: T_g(X).flat[i] == X.flat[source_cell(H, W, g, i)].
// Requires valid(H, W, g) and 0 <= i < H*W; the result is in [0, H*W).
MSSYM_HD inline int source_cell(int H, int W, unsigned g, int i) {
  int r = i / W, c = i - r * W;
  if (g & 1u) r = H - 1 - r;  // the steps of T_g, last one first
  if (g & 2u) c = W - 1 - c;
  return (g & 4u) ? c * W + r : r * W + c;
}

// The body of ms_sym_cell_map_host (mssym.hip adds the error message): writes H*W entries and
// returns 0, or writes nothing and returns 1 for a bad shape (max_cells: MS_AVOID_MAX_CELLS), an
// invalid g or a null map.
inline int cell_map_host(int H, int W, int g, int* map, int max_cells) {
  if (H < 1 || W < 1 || H > max_cells || W > max_cells || H * W > max_cells) return 1;
  if (!map || g < 0 || !valid(H, W, (unsigned)g)) return 1;
  for (int i = 0; i < H * W; ++i) map[i] = source_cell(H, W, (unsigned)g, i);
  return 0;
}

}  // namespace mssym

#endif  // MSSYM_MAP_H
