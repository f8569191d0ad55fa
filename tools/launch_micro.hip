// Micro-benchmark (tools only): launch/latency floors for the env-step shapes.
// Times graph-replayed launch sequences with hipEvents; run under
// `rocprofv3 --kernel-trace --stats` for per-kernel durations.
//   hipcc -O3 --offload-arch=gfx950 -o /tmp/launch_micro tools/launch_micro.hip
// `launch_micro forms` prices the store forms of the obs-shaped kernel instead
// (plain / nt / write-through; profiles/r07/store_policy_micro.txt).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CK(x)                                                                 \
  do {                                                                        \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) {                                                   \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      exit(1);                                                                \
    }                                                                         \
  } while (0)

__global__ __launch_bounds__(64) void k_null64(int64_t* out) {
  if (threadIdx.x == 0) out[blockIdx.x] = blockIdx.x;
}
__global__ __launch_bounds__(256) void k_null256(int64_t* out) {
  if ((threadIdx.x & 63) == 0) out[blockIdx.x * 4 + (threadIdx.x >> 6)] = blockIdx.x;
}
// one read of 64 B per env (lane-per-row words), one 8-B write
__global__ __launch_bounds__(64) void k_rw64(const uint64_t* rows, int64_t* out) {
  const int lane = threadIdx.x;
  uint64_t v = lane < 4 ? rows[blockIdx.x * 4 + lane] : 0;
  v = __ballot(v != 0);
  if (lane == 0) out[blockIdx.x] = (int64_t)v;
}
// obs-shaped store: 10 float4 per lane per env (10 KiB per env), 1 wave per env
__global__ __launch_bounds__(64) void k_store64(float4* obs) {
  float4* o = obs + (size_t)blockIdx.x * 640 + threadIdx.x;
  const float f = (float)(threadIdx.x & 1);
#pragma unroll
  for (int c = 0; c < 10; ++c) o[c * 64] = make_float4(f, 0.f, f, 0.f);
}
// same bytes, 4 envs per 256-thread workgroup
__global__ __launch_bounds__(256) void k_store256(float4* obs) {
  const int env = blockIdx.x * 4 + (threadIdx.x >> 6);
  float4* o = obs + (size_t)env * 640 + (threadIdx.x & 63);
  const float f = (float)(threadIdx.x & 1);
#pragma unroll
  for (int c = 0; c < 10; ++c) o[c * 64] = make_float4(f, 0.f, f, 0.f);
}


// ---- store-form variants of k_store256: same bytes, 16-B vector stores only ----
// 0 plain, 1 non-temporal (nt), 2 write-through (sc1), 3 sc0 sc1, 4 write-through as a
// buffer store through a per-env resource (plane offsets fold into the immediate)
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
enum { F_PLAIN = 0, F_NT = 1, F_SC1 = 2, F_SC0SC1 = 3, F_BUF_SC1 = 4, F_COUNT = 5 };
static const char* const kFormName[F_COUNT] = {"(a) plain", "(b) nt", "(c) sc1", "(d) sc0 sc1", "(c') buffer sc1"};

template <int FORM>
__device__ __forceinline__ void st16(float4* p, f32x4_t x) {
  if constexpr (FORM == F_NT) {
    __builtin_nontemporal_store(x, reinterpret_cast<f32x4_t*>(p));
  } else if constexpr (FORM == F_SC1) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1"
                 :
                 : "v"((__attribute__((address_space(1))) f32x4_t*)p), "v"(x)
                 : "memory");
  } else if constexpr (FORM == F_SC0SC1) {
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1"
                 :
                 : "v"((__attribute__((address_space(1))) f32x4_t*)p), "v"(x)
                 : "memory");
  } else {
    *reinterpret_cast<f32x4_t*>(p) = x;
  }
}

template <int FORM>
__global__ __launch_bounds__(256) void k_store256f(float4* obs) {
  const int env = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int l = threadIdx.x & 63;
  const float f = (float)(threadIdx.x & 1);
  const f32x4_t x = {f, 0.f, f, 0.f};
  if constexpr (FORM == F_BUF_SC1) {
    // the env's 10 KiB as one buffer resource, built from wave-uniform words; a store past
    // its 10240 records would be dropped by the range check
    const uint64_t b = (uint64_t)(obs + (size_t)env * 640);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32));
    auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0, 10240, 0x00020000);
    const u32x4_t u = {__float_as_uint(f), 0u, __float_as_uint(f), 0u};
#pragma unroll
    for (int c = 0; c < 10; ++c) __builtin_amdgcn_raw_buffer_store_b128(u, rsrc, l * 16 + c * 1024, 0, 16);
  } else {
    float4* o = obs + (size_t)env * 640 + l;
#pragma unroll
    for (int c = 0; c < 10; ++c) st16<FORM>(o + c * 64, x);
  }
}

typedef void (*Launch)(hipStream_t, void*, void*, int);

static float time_graph(hipStream_t s, Launch fn, void* a, void* b, int n, int reps) {
  hipGraph_t g;
  hipGraphExec_t ge;
  CK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
  for (int i = 0; i < reps; ++i) fn(s, a, b, n);
  CK(hipStreamEndCapture(s, &g));
  CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
  CK(hipGraphLaunch(ge, s));  // warm
  CK(hipStreamSynchronize(s));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  CK(hipEventRecord(e0, s));
  CK(hipGraphLaunch(ge, s));
  CK(hipEventRecord(e1, s));
  CK(hipEventSynchronize(e1));
  float ms;
  CK(hipEventElapsedTime(&ms, e0, e1));
  CK(hipGraphExecDestroy(ge));
  CK(hipGraphDestroy(g));
  return ms * 1000.f / reps;
}

static void L_null64(hipStream_t s, void* a, void*, int n) { k_null64<<<n, 64, 0, s>>>((int64_t*)a); }
static void L_null256(hipStream_t s, void* a, void*, int n) { k_null256<<<n / 4, 256, 0, s>>>((int64_t*)a); }
static void L_rw64(hipStream_t s, void* a, void* b, int n) { k_rw64<<<n, 64, 0, s>>>((const uint64_t*)b, (int64_t*)a); }
static void L_store64(hipStream_t s, void* a, void* b, int n) { k_store64<<<n, 64, 0, s>>>((float4*)b); }
static void L_store256(hipStream_t s, void* a, void* b, int n) { k_store256<<<n / 4, 256, 0, s>>>((float4*)b); }


// The store-form launches walk a ring of obs slots larger than the 256 MiB Infinity Cache
// twice over (as bench.py's obs ring), so no launch finds its lines cached from the last pass.
static const size_t kRingBytes = (size_t)16 * 4096 * 10240;  // 640 MiB
static int g_slot = 0;
template <int FORM>
static void L_form(hipStream_t s, void*, void* b, int n) {
  const int nslots = (int)(kRingBytes / ((size_t)n * 10240));
  float4* o = (float4*)b + (size_t)(g_slot++ % nslots) * n * 640;
  k_store256f<FORM><<<n / 4, 256, 0, s>>>(o);
}
template <int FORM>
static void L_form_null(hipStream_t s, void* a, void* b, int n) {
  L_form<FORM>(s, a, b, n);
  k_null256<<<n / 4, 256, 0, s>>>((int64_t*)a);
}

static void store_forms(hipStream_t s, void* a, void* ring, int reps) {
  static const Launch one[F_COUNT] = {L_form<0>, L_form<1>, L_form<2>, L_form<3>, L_form<4>};
  static const Launch pair[F_COUNT] = {L_form_null<0>, L_form_null<1>, L_form_null<2>, L_form_null<3>,
                                       L_form_null<4>};
  const int ns[] = {4096, 32768};
  printf("store forms, k_store256 shape (10 KiB per wave, 4 waves per workgroup), 640 MiB ring, us per launch\n");
  printf("  span = graph of the store kernel alone; +boundary = graph of (store, null) pairs minus graph of null\n");
  for (int n : ns) {
    const double mb = (double)n * 10240 / 1e6;
    printf("n=%d (%.1f MB per launch)\n", n, mb);
    for (int pass = 0; pass < 3; ++pass) {  // three passes, forms interleaved inside each
      const float tnull = time_graph(s, L_null256, a, ring, n, reps);
      printf("  pass %d  null %6.2f\n", pass, tnull);
      for (int f = 0; f < F_COUNT; ++f) {
        g_slot = 0;
        const float t1 = time_graph(s, one[f], a, ring, n, reps);
        g_slot = 0;
        const float t2 = time_graph(s, pair[f], a, ring, n, reps);
        printf("    %-16s span %7.2f (%5.0f GB/s)   +boundary %7.2f\n", kFormName[f], t1, mb / t1 * 1e3, t2 - tnull);
      }
    }
  }
}

int main(int argc, char** argv) {
  const int reps = 200;
  hipStream_t s;
  CK(hipStreamCreate(&s));
  void *a, *b;
  CK(hipMalloc(&a, 32768 * 8 * 4));
  CK(hipMalloc(&b, (size_t)32768 * 640 * 16));
  CK(hipMemset(b, 1, (size_t)32768 * 640 * 16));
  if (argc > 1 && !strcmp(argv[1], "forms")) {
    void* ring;
    CK(hipMalloc(&ring, kRingBytes));
    CK(hipMemset(ring, 1, kRingBytes));
    store_forms(s, a, ring, reps);
    return 0;
  }
  const int ns[] = {4096, 32768};
  for (int n : ns) {
    printf("n=%d\n", n);
    printf("  null 1 wave/WG        %7.2f us\n", time_graph(s, L_null64, a, b, n, reps));
    printf("  null 4 waves/WG       %7.2f us\n", time_graph(s, L_null256, a, b, n, reps));
    printf("  read64B+write8B/env   %7.2f us\n", time_graph(s, L_rw64, a, b, n, reps));
    const float t64 = time_graph(s, L_store64, a, b, n, reps);
    const float t256 = time_graph(s, L_store256, a, b, n, reps);
    const double mb = (double)n * 10240 / 1e6;
    printf("  store 10KiB/env 1w/WG %7.2f us  (%.0f GB/s)\n", t64, mb / t64 * 1e3);
    printf("  store 10KiB/env 4w/WG %7.2f us  (%.0f GB/s)\n", t256, mb / t256 * 1e3);
  }
  return 0;
}
