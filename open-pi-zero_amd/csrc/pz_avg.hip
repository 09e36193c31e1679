// Weight averaging over the flat parameter arena (EMA / SWA: the reference's src/agent/model_averaging.py, which
// drives torch.optim.swa_utils.AveragedModel): avg <- lerp(avg, p, w) and an in-place exchange of two buffers.
//
// Both are pure HBM streams (lerp: 2 reads + 1 write of 2 B per element, swap: 2 + 2), so the whole design is the
// access pattern: 16 B per lane, every load of a tile issued before the first use (AVG_U vectors of each operand:
// 8 independent 16-byte loads in flight per lane), a persistent grid of at most AVG_MAX_BLOCKS workgroups striding
// over 16 KiB tiles, nontemporal loads and stores (every byte is touched once per launch and the arena is 25 x the
// Infinity Cache).  Elements past the last whole 16-byte vector (n % 8) are handled one per lane by workgroup 0.
// Deterministic: every element is written by exactly one lane, no atomics.
//
// pz_avg_lerp reproduces torch.lerp's bf16 kernel bit for bit: fp32 a, x, d = x - a, then
//   w < 0.5 ? fma(w, d, a) : fma(-d, 1 - w, x)        (ATen/native/Lerp.h)
// rounded to bf16 with round-to-nearest-even.  The FMAs are explicit and the file is built with -ffp-contract=off:
// the unfused a + w * d differs from torch in a few elements per million.
#include "pz_common.h"

#ifndef PZ_AVG_NT
#define PZ_AVG_NT 1  // 0: plain loads / stores (A/B builds only)
#endif

namespace {

constexpr int AVG_THREADS = 256;
constexpr int AVG_U = 4;                                      // 16-byte vectors per lane and operand per tile
constexpr int64_t AVG_TILE_VEC = (int64_t)AVG_THREADS * AVG_U;  // 1024 vectors = 16 KiB per operand
constexpr int64_t AVG_MAX_BLOCKS = 2048;                      // 256 CUs x 8 resident workgroups

__device__ __forceinline__ u32x4 ld16(const u32x4* p) {
#if PZ_AVG_NT
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}
__device__ __forceinline__ void st16(u32x4* p, u32x4 v) {
#if PZ_AVG_NT
  __builtin_nontemporal_store(v, p);
#else
  *p = v;
#endif
}

template <bool LOW>  // LOW: |w| < 0.5
__device__ __forceinline__ float lerp1(float a, float x, float w, float omw) {
  const float d = __fsub_rn(x, a);
  return LOW ? __fmaf_rn(w, d, a) : __fmaf_rn(-d, omw, x);
}

template <bool LOW>
__device__ __forceinline__ u32x4 lerp8(u32x4 av, u32x4 xv, float w, float omw) {
  u32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float lo = lerp1<LOW>(__uint_as_float(av[k] << 16), __uint_as_float(xv[k] << 16), w, omw);
    const float hi = lerp1<LOW>(__uint_as_float(av[k] & 0xffff0000u), __uint_as_float(xv[k] & 0xffff0000u), w, omw);
    o[k] = pack2bf(lo, hi);
  }
  return o;
}

template <bool LOW>
__global__ void __launch_bounds__(AVG_THREADS) avg_lerp_kernel(bf16_t* __restrict__ avg, const bf16_t* __restrict__ p,
                                                               int64_t n, float w, float omw) {
  const int64_t nvec = n >> 3;
  u32x4* A = reinterpret_cast<u32x4*>(avg);
  const u32x4* P = reinterpret_cast<const u32x4*>(p);
  for (int64_t t0 = (int64_t)blockIdx.x * AVG_TILE_VEC; t0 < nvec; t0 += (int64_t)gridDim.x * AVG_TILE_VEC) {
    const int64_t i0 = t0 + threadIdx.x;
    u32x4 av[AVG_U], xv[AVG_U];
    if (t0 + AVG_TILE_VEC <= nvec) {  // whole tile (workgroup-uniform): all loads, then all stores
#pragma unroll
      for (int u = 0; u < AVG_U; ++u) av[u] = ld16(A + i0 + u * AVG_THREADS);
#pragma unroll
      for (int u = 0; u < AVG_U; ++u) xv[u] = ld16(P + i0 + u * AVG_THREADS);
#pragma unroll
      for (int u = 0; u < AVG_U; ++u) st16(A + i0 + u * AVG_THREADS, lerp8<LOW>(av[u], xv[u], w, omw));
    } else {
#pragma unroll
      for (int u = 0; u < AVG_U; ++u) {
        const int64_t i = i0 + u * AVG_THREADS;
        if (i < nvec) st16(A + i, lerp8<LOW>(ld16(A + i), ld16(P + i), w, omw));
      }
    }
  }
  const int64_t e = (nvec << 3) + threadIdx.x;  // scalar tail: n % 8 elements
  if (blockIdx.x == 0 && e < n) avg[e] = f2bf(lerp1<LOW>(bf2f(avg[e]), bf2f(p[e]), w, omw));
}

__global__ void __launch_bounds__(AVG_THREADS) avg_swap_kernel(bf16_t* __restrict__ a, bf16_t* __restrict__ b,
                                                               int64_t n) {
  const int64_t nvec = n >> 3;
  u32x4* A = reinterpret_cast<u32x4*>(a);
  u32x4* B = reinterpret_cast<u32x4*>(b);
  for (int64_t t0 = (int64_t)blockIdx.x * AVG_TILE_VEC; t0 < nvec; t0 += (int64_t)gridDim.x * AVG_TILE_VEC) {
    const int64_t i0 = t0 + threadIdx.x;
    u32x4 av[AVG_U], bv[AVG_U];
    if (t0 + AVG_TILE_VEC <= nvec) {
#pragma unroll
      for (int u = 0; u < AVG_U; ++u) av[u] = ld16(A + i0 + u * AVG_THREADS);
#pragma unroll
      for (int u = 0; u < AVG_U; ++u) bv[u] = ld16(B + i0 + u * AVG_THREADS);
#pragma unroll
      for (int u = 0; u < AVG_U; ++u) st16(A + i0 + u * AVG_THREADS, bv[u]);
#pragma unroll
      for (int u = 0; u < AVG_U; ++u) st16(B + i0 + u * AVG_THREADS, av[u]);
    } else {
#pragma unroll
      for (int u = 0; u < AVG_U; ++u) {
        const int64_t i = i0 + u * AVG_THREADS;
        if (i < nvec) {
          const u32x4 x = ld16(A + i), y = ld16(B + i);
          st16(A + i, y);
          st16(B + i, x);
        }
      }
    }
  }
  const int64_t e = (nvec << 3) + threadIdx.x;
  if (blockIdx.x == 0 && e < n) {
    const bf16_t x = a[e], y = b[e];
    a[e] = y;
    b[e] = x;
  }
}

inline unsigned avg_grid(int64_t n) {
  const int64_t tiles = ((n >> 3) + AVG_TILE_VEC - 1) / AVG_TILE_VEC;
  return (unsigned)(tiles < 1 ? 1 : (tiles < AVG_MAX_BLOCKS ? tiles : AVG_MAX_BLOCKS));
}

// [a, a + 2n) and [b, b + 2n) bytes share no byte
inline bool avg_disjoint(const void* a, const void* b, int64_t n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, len = (uintptr_t)n * 2;
  return x + len <= y || y + len <= x;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int pz_avg_lerp(void* avg, const void* p, int64_t n, float w, void* stream) {
  PZ_CHECK_ARG(avg && p, "avg_lerp: null pointer");
  PZ_CHECK_ARG(n > 0, "avg_lerp: n must be positive");
  PZ_CHECK_ARG(PZ_ALIGNED(avg, 16) && PZ_ALIGNED(p, 16), "avg_lerp: pointers must be 16-byte aligned");
  PZ_CHECK_ARG(avg_disjoint(avg, p, n), "avg_lerp: avg and p overlap");
  const float omw = 1.0f - w;
  if (fabsf(w) < 0.5f)
    hipLaunchKernelGGL(avg_lerp_kernel<true>, dim3(avg_grid(n)), dim3(AVG_THREADS), 0, ST, (bf16_t*)avg,
                       (const bf16_t*)p, n, w, omw);
  else
    hipLaunchKernelGGL(avg_lerp_kernel<false>, dim3(avg_grid(n)), dim3(AVG_THREADS), 0, ST, (bf16_t*)avg,
                       (const bf16_t*)p, n, w, omw);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}

extern "C" int pz_avg_swap(void* a, void* b, int64_t n, void* stream) {
  PZ_CHECK_ARG(a && b, "avg_swap: null pointer");
  PZ_CHECK_ARG(n > 0, "avg_swap: n must be positive");
  PZ_CHECK_ARG(PZ_ALIGNED(a, 16) && PZ_ALIGNED(b, 16), "avg_swap: pointers must be 16-byte aligned");
  PZ_CHECK_ARG(avg_disjoint(a, b, n), "avg_swap: a and b overlap");
  hipLaunchKernelGGL(avg_swap_kernel, dim3(avg_grid(n)), dim3(AVG_THREADS), 0, ST, (bf16_t*)a, (bf16_t*)b, n);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}
