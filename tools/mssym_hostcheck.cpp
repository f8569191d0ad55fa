// Stand-alone check of the symmetry cell map (minesweeper-ppo_amd/csrc/mssym_map.h, the function
// every kernel of mssym.hip and ms_sym_cell_map_host use): every shape of up to 512 cells with
// H, W <= 64 and random larger ones, every valid g, the map written into an exactly-sized heap
// buffer and read from an exactly-sized plane, so that a sanitizer sees any index outside
// [0, H*W). Each map is checked against the three steps of include/mssym.h applied one after the
// other to a plane of cell numbers, to be a permutation, and to be undone by inverse(g).
// Plain C++, so it runs under sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iminesweeper-ppo_amd/csrc tools/mssym_hostcheck.cpp -o tools/bin/mssym_hostcheck
//   tools/bin/mssym_hostcheck
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "mssym_map.h"

// the body of ms_sym_cell_map_host (mssym::cell_map_host), on an exactly-sized buffer
static std::vector<int> cell_map(int H, int W, unsigned g) {
  std::vector<int> map((size_t)(H * W), -1);
  if (mssym::cell_map_host(H, W, (int)g, map.data(), 512)) {
    printf("REFUSED: %dx%d g %u\n", H, W, g);
    exit(1);
  }
  return map;
}

// the definition, once more: transpose, reverse the rows, reverse the columns, as whole planes
static std::vector<int> by_steps(int H, int W, unsigned g) {
  std::vector<int> x((size_t)(H * W)), y((size_t)(H * W));
  for (int i = 0; i < H * W; ++i) x[(size_t)i] = i;
  if (g & 4u) {
    for (int r = 0; r < H; ++r)
      for (int c = 0; c < W; ++c) y[(size_t)(r * W + c)] = x[(size_t)(c * W + r)];
    x = y;
  }
  if (g & 1u) {
    for (int r = 0; r < H; ++r)
      for (int c = 0; c < W; ++c) y[(size_t)(r * W + c)] = x[(size_t)((H - 1 - r) * W + c)];
    x = y;
  }
  if (g & 2u) {
    for (int r = 0; r < H; ++r)
      for (int c = 0; c < W; ++c) y[(size_t)(r * W + c)] = x[(size_t)(r * W + W - 1 - c)];
    x = y;
  }
  return x;
}

static int check_shape(int H, int W, long* maps) {
  const int A = H * W;
  for (unsigned g = 0; g < 8; ++g) {
    if (mssym::valid(H, W, g) != (g < 4 || H == W)) {
      printf("WRONG valid(): %dx%d g %u\n", H, W, g);
      return 1;
    }
    if (!mssym::valid(H, W, g)) continue;
    const std::vector<int> map = cell_map(H, W, g), want = by_steps(H, W, g);
    const std::vector<int> back = cell_map(H, W, mssym::inverse(g));
    std::vector<char> seen((size_t)A, 0);
    std::vector<int> plane((size_t)A);
    for (int i = 0; i < A; ++i) plane[(size_t)i] = 1000 + i;
    for (int i = 0; i < A; ++i) {
      const int s = map[(size_t)i];
      if (s != want[(size_t)i] || plane[(size_t)s] != 1000 + s || seen[(size_t)s]++ ||
          map[(size_t)back[(size_t)i]] != i) {
        printf("WRONG MAP: %dx%d g %u cell %d -> %d (want %d)\n", H, W, g, i, s, want[(size_t)i]);
        return 1;
      }
    }
    *maps += 1;
  }
  if (mssym::valid(H, W, 8u) || mssym::valid(H, W, 255u) || mssym::inverse(mssym::inverse(5u)) != 5u ||
      mssym::inverse(5u) != 6u || mssym::inverse(4u) != 4u || mssym::inverse(7u) != 7u || mssym::inverse(3u) != 3u) {
    printf("WRONG valid() or inverse()\n");
    return 1;
  }
  int one = -7;  // refused calls write nothing
  if (!mssym::cell_map_host(H, W, 8, &one, 512) || !mssym::cell_map_host(H, W, -1, &one, 512) ||
      !mssym::cell_map_host(H, W, 0, nullptr, 512) || !mssym::cell_map_host(0, W, 0, &one, 512) ||
      !mssym::cell_map_host(H, 513, 0, &one, 512) || (H != W && !mssym::cell_map_host(H, W, 4, &one, 512)) ||
      one != -7) {
    printf("A BAD CALL WAS ACCEPTED: %dx%d\n", H, W);
    return 1;
  }
  return 0;
}

int main() {
  long shapes = 0, maps = 0;
  for (int H = 1; H <= 64; ++H)
    for (int W = 1; W <= 64 && H * W <= 512; ++W, ++shapes)
      if (check_shape(H, W, &maps)) return 1;
  std::mt19937 rng(1);
  for (int it = 0; it < 400; ++it, shapes += 2) {
    const int H = 1 + (int)(rng() % 512u), W = 1 + (int)(rng() % (unsigned)(512 / H));
    if (check_shape(H, W, &maps) || check_shape(W, H, &maps)) return 1;
  }
  printf("ok: %ld shapes of up to 512 cells, %ld maps\n", shapes, maps);
  return 0;
}
