// 4-bit base weights of QLoRA (quantize: True): blockwise fp4 / nf4 codes in blocks of 64 with
// double-quantised block scales -- the public storage format of bitsandbytes 0.45, restated in tests/quant4_ref.py.
//
//   pz_q4_quantize   bf16 [n] -> packed codes uint8 [n / 2] (even index in the high nibble) + fp32 absmax per block.
//                    Once per Linear at load: one wave per block, lane = element.  x = fp32(fp16(bf16 w));
//                    absmax = max |x|; xn = x * (1 / absmax) (IEEE division, 0 for a zero block); the code is the
//                    count of fp32 midpoints of the sorted table below xn (fp4: on |xn|, sign bit = xn < 0).
//   pz_q4_dequant    the per-step hot path, up to PZ_Q4_MAX_SEGS weights (q|k|v, gate|up) in one launch:
//                    absmax' = qmap[code8] * nested_absmax + offset once per 8-weight chunk (8 chunks per block),
//                    w = bf16(fp16(table[nibble] * absmax')).  A streaming kernel: every lane reads 4 packed bytes and
//                    writes one 16-byte bf16 vector, so a wave reads 256 B and writes 1 KiB contiguously per instruction,
//                    four chunks per lane in flight; the 256-entry map and the 16-entry table sit in LDS.  No atomics,
//                    no per-element branches.
//
// Every product and sum is rounded by itself: the file is built with -ffp-contract=off (build_native.py) and without
// fast-math, so the numpy restatement gives the same bits.
#include "pz_common.h"

namespace {

constexpr int Q4_THREADS = 256;
constexpr int Q4_UNROLL = 4;                              // chunks per lane
constexpr int64_t Q4_TILE = Q4_THREADS * Q4_UNROLL * 8;  // weights per workgroup

// [table id][code]: fp4 (bit 3 = sign), nf4 (ascending)
__constant__ float Q4_TABLE[2][16] = {
    {0.f, 0.0052083333f, 0.66666667f, 1.f, 0.33333333f, 0.5f, 0.16666667f, 0.25f, -0.f, -0.0052083333f, -0.66666667f,
     -1.f, -0.33333333f, -0.5f, -0.16666667f, -0.25f},
    {-1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f, -0.28444138169288635f,
     -0.18477343022823334f, -0.09105003625154495f, 0.0f, 0.07958029955625534f, 0.16093020141124725f,
     0.24611230194568634f, 0.33791524171829224f, 0.44070982933044434f, 0.5626170039176941f, 0.7229568362236023f, 1.0f}};
// fp4 codes in ascending order of magnitude
__constant__ int Q4_FP4_ORDER[8] = {0, 1, 6, 7, 4, 5, 2, 3};

__device__ __forceinline__ float to_half_and_back(float f) { return (float)(_Float16)f; }

// w = fp32(fp16(t * am)): the fp32 product rounded by itself, then to fp16.  The empty asm keeps the compiler from
// fusing the two into v_fma_mixlo_f16 (t * am + 0, which turns the -0 of fp4's code 8 into +0).
__device__ __forceinline__ float q4_weight(float t, float am) {
  float p = t * am;
  asm volatile("" : "+v"(p));
  return to_half_and_back(p);
}

__global__ void __launch_bounds__(Q4_THREADS) q4_quantize_kernel(const bf16_t* __restrict__ w,
                                                                uint8_t* __restrict__ packed,
                                                                float* __restrict__ absmax, int64_t n, int64_t nb,
                                                                int table) {
  const int lane = threadIdx.x & 63;
  const int64_t blk = (int64_t)blockIdx.x * (Q4_THREADS / 64) + (threadIdx.x >> 6);
  if (blk >= nb) return;  // whole waves leave together: the shuffles below see full waves
  const int64_t i = blk * 64 + lane;
  const float x = i < n ? to_half_and_back(bf2f(w[i])) : 0.f;
  const float am = warp_max(fabsf(x));
  const float inv = am > 0.f ? 1.f / am : 0.f;
  const float xn = x * inv;
  int code;
  if (table == 0) {
    const float a = fabsf(xn);
    int rank = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      const float mid = (Q4_TABLE[0][Q4_FP4_ORDER[j]] + Q4_TABLE[0][Q4_FP4_ORDER[j + 1]]) * 0.5f;
      rank += a > mid ? 1 : 0;
    }
    code = Q4_FP4_ORDER[rank] | (xn < 0.f ? 8 : 0);
  } else {
    code = 0;
#pragma unroll
    for (int j = 0; j < 15; ++j) {
      const float mid = (Q4_TABLE[1][j] + Q4_TABLE[1][j + 1]) * 0.5f;
      code += xn > mid ? 1 : 0;
    }
  }
  const int nxt = __shfl_down(code, 1, 64);
  if (!(lane & 1) && i < n) packed[i >> 1] = (uint8_t)((code << 4) | nxt);  // n is even: i + 1 < n too
  if (lane == 0) absmax[blk] = am;
}

struct Q4Seg {
  const uint8_t* packed;
  const uint8_t* codes;
  const float* nam;
  bf16_t* dst;
  int64_t n;
  int64_t tile0;  // first workgroup of this segment
  float offset;
};
struct Q4Segs {
  Q4Seg s[PZ_Q4_MAX_SEGS];
  int count;
};

__global__ void __launch_bounds__(Q4_THREADS) q4_dequant_kernel(Q4Segs segs, const float* __restrict__ qmap,
                                                               int table) {
  __shared__ float s_map[256];
  __shared__ float s_tab[16];
  s_map[threadIdx.x] = qmap[threadIdx.x];
  if (threadIdx.x < 16) s_tab[threadIdx.x] = Q4_TABLE[table][threadIdx.x];
  __syncthreads();
  int si = 0;
#pragma unroll
  for (int k = 1; k < PZ_Q4_MAX_SEGS; ++k)
    if (k < segs.count && (int64_t)blockIdx.x >= segs.s[k].tile0) si = k;
  const Q4Seg& sg = segs.s[si];
  const int64_t n = sg.n;
  const int64_t base = ((int64_t)blockIdx.x - sg.tile0) * Q4_TILE;
  const uint8_t* __restrict__ pk = sg.packed;
  bf16_t* __restrict__ dst = sg.dst;
#pragma unroll
  for (int u = 0; u < Q4_UNROLL; ++u) {
    const int64_t e0 = base + ((int64_t)u * Q4_THREADS + threadIdx.x) * 8;
    if (e0 >= n) continue;
    const int64_t blk = e0 >> 6;
    const float am = s_map[sg.codes[blk]] * sg.nam[blk >> 8] + sg.offset;
    if (e0 + 8 <= n) {
      const unsigned word = *(const unsigned*)(pk + (e0 >> 1));
      unsigned o[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const unsigned byte = (word >> (8 * b)) & 0xffu;
        const float hi = q4_weight(s_tab[byte >> 4], am);
        const float lo = q4_weight(s_tab[byte & 15u], am);
        o[b] = pack2bf(hi, lo);  // the even element (high nibble) at the lower address
      }
      *(u32x4*)(dst + e0) = u32x4{o[0], o[1], o[2], o[3]};
    } else {  // the ragged end of a weight whose size is no multiple of 8 (n is even)
      for (int64_t e = e0; e < n; e += 2) {
        const unsigned byte = pk[e >> 1];
        dst[e] = f2bf(q4_weight(s_tab[byte >> 4], am));
        dst[e + 1] = f2bf(q4_weight(s_tab[byte & 15u], am));
      }
    }
  }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int pz_q4_quantize(const void* w, void* packed, float* absmax, int64_t n, int32_t table, void* stream) {
  PZ_CHECK_ARG(w && packed && absmax, "q4_quantize: null pointer");
  PZ_CHECK_ARG(table == PZ_Q4_FP4 || table == PZ_Q4_NF4, "q4_quantize: table %d is neither fp4 (0) nor nf4 (1)",
               (int)table);
  PZ_CHECK_ARG(n > 0 && n % 2 == 0, "q4_quantize: n = %lld must be positive and even (two codes per byte)",
               (long long)n);
  const int64_t nb = (n + 63) / 64;
  const int64_t wgs = (nb + Q4_THREADS / 64 - 1) / (Q4_THREADS / 64);
  PZ_CHECK_ARG(wgs <= 0x7fffffffLL, "q4_quantize: n = %lld is too large for one launch", (long long)n);
  hipLaunchKernelGGL(q4_quantize_kernel, dim3((unsigned)wgs), dim3(Q4_THREADS), 0, ST, (const bf16_t*)w,
                     (uint8_t*)packed, absmax, n, nb, (int)table);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}

extern "C" int pz_q4_dequant_multi(const pz_q4_seg* segs, int32_t count, const float* qmap, int32_t table,
                                   void* stream) {
  PZ_CHECK_ARG(segs && qmap, "q4_dequant: null pointer");
  PZ_CHECK_ARG(count >= 1 && count <= PZ_Q4_MAX_SEGS, "q4_dequant: %d segments, 1..%d are taken", (int)count,
               PZ_Q4_MAX_SEGS);
  PZ_CHECK_ARG(table == PZ_Q4_FP4 || table == PZ_Q4_NF4, "q4_dequant: table %d is neither fp4 (0) nor nf4 (1)",
               (int)table);
  Q4Segs k;
  k.count = count;
  int64_t tiles = 0;
  for (int i = 0; i < count; ++i) {
    const pz_q4_seg& s = segs[i];
    PZ_CHECK_ARG(s.packed && s.absmax_codes && s.nested_absmax && s.dst, "q4_dequant: null pointer in segment %d", i);
    PZ_CHECK_ARG(s.n > 0 && s.n % 2 == 0, "q4_dequant: n = %lld must be positive and even (two codes per byte)",
                 (long long)s.n);
    PZ_CHECK_ARG(PZ_ALIGNED(s.packed, 4) && PZ_ALIGNED(s.dst, 16),
                 "q4_dequant: packed must be 4-byte and dst 16-byte aligned (segment %d)", i);
    k.s[i] = Q4Seg{(const uint8_t*)s.packed, (const uint8_t*)s.absmax_codes, s.nested_absmax, (bf16_t*)s.dst, s.n,
                   tiles, s.offset};
    tiles += (s.n + Q4_TILE - 1) / Q4_TILE;
  }
  for (int i = count; i < PZ_Q4_MAX_SEGS; ++i) k.s[i] = Q4Seg{nullptr, nullptr, nullptr, nullptr, 0, tiles, 0.f};
  PZ_CHECK_ARG(tiles <= 0x7fffffffLL, "q4_dequant: too many elements for one launch");
  hipLaunchKernelGGL(q4_dequant_kernel, dim3((unsigned)tiles), dim3(Q4_THREADS), 0, ST, k, qmap, (int)table);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}

extern "C" int pz_q4_dequant(const void* packed, const void* absmax_codes, const float* nested_absmax, float offset,
                             const float* qmap, int32_t table, int64_t n, void* dst, void* stream) {
  const pz_q4_seg s = {packed, absmax_codes, nested_absmax, dst, n, offset};
  return pz_q4_dequant_multi(&s, 1, qmap, table, stream);
}
