// numpy's PCG64 as the env kernels run it (device, wave-uniform) and its host twin, which
// seeds the per-env streams (ms_create) and the late-start generator; plus splitmix64, the
// keyed hash of the tape policy, the sampler and the dropout masks. The two halves must
// produce the same stream, so they stand side by side. Internal to libmsenv.so.
#ifndef MSENV_PCG_H
#define MSENV_PCG_H

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace {

// ---------------------------------------------------------------------------
// numpy PCG64 (setseq_128 XSL-RR) + bounded Lemire draw, wave-uniform.
// ---------------------------------------------------------------------------
struct Pcg {
  uint64_t hi, lo, ihi, ilo;
  uint32_t has32, uinteger;
};

__device__ __forceinline__ void pcg_step(Pcg& r) {
  constexpr uint64_t MH = 0x2360ED051FC65DA4ull, ML = 0x4385DF649FCCF645ull;
  const uint64_t lo = r.lo * ML;
  uint64_t hi = __umul64hi(r.lo, ML) + r.lo * MH + r.hi * ML;
  const uint64_t lo2 = lo + r.ilo;
  hi += r.ihi + (lo2 < lo ? 1ull : 0ull);
  r.lo = lo2;
  r.hi = hi;
}

__device__ __forceinline__ uint64_t pcg_next64(Pcg& r) {
  pcg_step(r);
  const uint64_t v = r.hi ^ r.lo;
  const unsigned rot = (unsigned)(r.hi >> 58);
  return (v >> rot) | (v << ((64u - rot) & 63u));
}

__device__ __forceinline__ uint32_t pcg_next32(Pcg& r) {
  if (r.has32) {
    r.has32 = 0;
    return r.uinteger;
  }
  const uint64_t x = pcg_next64(r);
  r.has32 = 1;
  r.uinteger = (uint32_t)(x >> 32);
  return (uint32_t)x;
}

// random_bounded_uint64(0, j) for j < 2^32-1: numpy's buffered Lemire.
__device__ __forceinline__ uint32_t pcg_bounded(Pcg& r, uint32_t j) {
  if (j == 0) return 0;
  const uint32_t excl = j + 1u;
  uint64_t m = (uint64_t)pcg_next32(r) * excl;
  uint32_t left = (uint32_t)m;
  if (left < excl) {
    const uint32_t thr = (0xffffffffu - j) % excl;
    while (left < thr) {
      m = (uint64_t)pcg_next32(r) * excl;
      left = (uint32_t)m;
    }
  }
  return (uint32_t)(m >> 32);
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// numpy SeedSequence -> PCG64 seeding, host side (bit_generator.pyx / pcg64.c).
struct HostPcg {
  unsigned __int128 state, inc;
  int has32;
  uint32_t uinteger;
};

inline void host_seed(HostPcg& r, uint64_t seed) {
  uint32_t ent[2];
  int ne = 0;
  if (seed == 0) ent[ne++] = 0;
  while (seed) {
    ent[ne++] = (uint32_t)seed;
    seed >>= 32;
  }
  uint32_t hc = 0x43b0d7e5u;
  auto hashmix = [&hc](uint32_t v) {
    v ^= hc;
    hc *= 0x931e8875u;
    v *= hc;
    return v ^ (v >> 16);
  };
  auto mix = [](uint32_t x, uint32_t y) {
    uint32_t r = 0xca01f9ddu * x - 0x4973f715u * y;
    return r ^ (r >> 16);
  };
  uint32_t pool[4];
  for (int i = 0; i < 4; ++i) pool[i] = hashmix(i < ne ? ent[i] : 0u);
  for (int s = 0; s < 4; ++s)
    for (int d = 0; d < 4; ++d)
      if (s != d) pool[d] = mix(pool[d], hashmix(pool[s]));
  uint32_t w32[8];
  uint32_t hb = 0x8b51f9ddu;
  for (int i = 0; i < 8; ++i) {
    uint32_t v = pool[i & 3] ^ hb;
    hb *= 0x58f38dedu;
    v *= hb;
    w32[i] = v ^ (v >> 16);
  }
  uint64_t w[4];
  for (int i = 0; i < 4; ++i) w[i] = (uint64_t)w32[2 * i] | ((uint64_t)w32[2 * i + 1] << 32);
  const unsigned __int128 M = ((unsigned __int128)0x2360ED051FC65DA4ull << 64) | 0x4385DF649FCCF645ull;
  const unsigned __int128 initstate = ((unsigned __int128)w[0] << 64) | w[1];
  const unsigned __int128 initseq = ((unsigned __int128)w[2] << 64) | w[3];
  r.inc = (initseq << 1) | 1u;
  r.state = 0;
  r.state = r.state * M + r.inc;
  r.state += initstate;
  r.state = r.state * M + r.inc;
  r.has32 = 0;
  r.uinteger = 0;
}

inline uint32_t host_next32(HostPcg& r) {
  if (r.has32) {
    r.has32 = 0;
    return r.uinteger;
  }
  const unsigned __int128 M = ((unsigned __int128)0x2360ED051FC65DA4ull << 64) | 0x4385DF649FCCF645ull;
  r.state = r.state * M + r.inc;
  const uint64_t hi = (uint64_t)(r.state >> 64), lo = (uint64_t)r.state;
  const unsigned rot = (unsigned)(hi >> 58);
  const uint64_t v = hi ^ lo;
  const uint64_t x = (v >> rot) | (v << ((64u - rot) & 63u));
  r.has32 = 1;
  r.uinteger = (uint32_t)(x >> 32);
  return (uint32_t)x;
}

inline uint32_t host_bounded(HostPcg& r, uint32_t j) {
  if (j == 0) return 0;
  const uint32_t excl = j + 1u;
  uint64_t m = (uint64_t)host_next32(r) * excl;
  uint32_t left = (uint32_t)m;
  if (left < excl) {
    const uint32_t thr = (0xffffffffu - j) % excl;
    while (left < thr) {
      m = (uint64_t)host_next32(r) * excl;
      left = (uint32_t)m;
    }
  }
  return (uint32_t)(m >> 32);
}

}  // namespace

#endif  // MSENV_PCG_H
