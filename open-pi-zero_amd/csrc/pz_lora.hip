// Rank-r weight gradient of a LoRA adapter (ABI 22):
//
//   out[j][d] (+)= alpha * sum_m P[m][j] * Q[m][d]        (transposed: out[d][j])
//
// dA = s v^T x ([r, in]: Q = x, P = v = dy B) and dB = s dy^T u ([out, r]: Q = dy, P = u = x A^T, transposed).
// Both reduce over all M rows (70 656 at the benched micro-batch) into a tiny output, so the work is dealt over
// (128-column slab of Q) x (fixed row range of M): every element of Q is read by exactly one workgroup, P (R <= 128
// columns) is re-read per column slab out of L2.  Each workgroup writes its fp32 [R][128] partial to the caller's
// workspace and a second kernel sums the row ranges in index order: no atomics, so two runs give identical bits,
// and the partition depends on (M, D, R) only.
//
// Both operands are "k-strided" for the MFMA (the reduction index m is the row of the stored matrices), so the
// [64 m][128] tiles are staged in LDS as stored and read through ds_read_b64_tr_b16, like the TN form of
// pz_gemm's 128-tile kernel (same image, same XOR swizzle).  256 threads = 4 waves, each 32 of the slab's 128
// columns x all RB * 16 adapter rows (acc[RB][2]); register-staged double buffering, one barrier per 64 rows.
#include "pz_common.h"

namespace {

constexpr int LT = 256;               // threads
constexpr int LK = 64;                // rows of M per step
constexpr int LD = 128;               // columns of Q per workgroup
constexpr int L_TILE = LK * 128 * 2;  // one [64][128] bf16 image
constexpr int64_t L_TARGET_WGS = 1024;
constexpr int64_t L_MAX_PARTS = 64;

__device__ __forceinline__ int lsw_tr(int k) { return ((k & 3) | (((k >> 3) & 1) << 2)) << 2; }

// rows [k0, k0 + 64) x 128 columns from col0 of a row-major bf16 matrix; rows >= kend and columns >= C read as zero
__device__ __forceinline__ void l_g2r(u32x4 (&r)[4], const bf16_t* __restrict__ base, int64_t ld, int64_t col0,
                                      int64_t C, int64_t k0, int64_t kend) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = t + LT * i;
    const int kr = c >> 4, rc = c & 15;
    const int64_t kk = k0 + kr, cc = col0 + 8 * rc;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (kk < kend && cc < C) v = *reinterpret_cast<const u32x4*>(base + kk * ld + cc);
    r[i] = v;
  }
}

__device__ __forceinline__ void l_r2s(const u32x4 (&r)[4], char* lds) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = t + LT * i;
    const int kr = c >> 4, rc = c & 15;
    *reinterpret_cast<u32x4*>(lds + kr * 256 + (((2 * rc) ^ lsw_tr(kr)) << 3)) = r[i];
  }
}

// MFMA fragment: image columns rb*16 + (lane & 15), k = kk*32 + 8*(lane >> 4) + j
__device__ __forceinline__ bf16x8 l_frag(const char* lds, int rb, int kk, int lane) {
  const int q = (lane & 15) >> 2, p = lane & 3;
  s16x8 out;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int k = kk * 32 + 8 * (lane >> 4) + 4 * t + q;
    const int off = k * 256 + (((4 * rb + p) ^ lsw_tr(k)) << 3);
    s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lds + off));
    out[4 * t + 0] = v[0];
    out[4 * t + 1] = v[1];
    out[4 * t + 2] = v[2];
    out[4 * t + 3] = v[3];
  }
  return __builtin_bit_cast(bf16x8, out);
}

struct LoraP {
  const bf16_t* Q;
  const bf16_t* P;
  bf16_t* out;
  float* ws;
  int64_t ldq, ldp, ld_out, M, D, R, rows_per_part;
  int nparts, transposed, beta;
  float alpha;
};

// grid (column slabs, parts): ws[part][j][d] = sum over the part's rows of P[m][j] Q[m][d]
template <int RB>
__global__ void __launch_bounds__(LT) lora_wgrad_kernel(LoraP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sQ = smem;               // [2][L_TILE]
  char* sP = smem + 2 * L_TILE;  // [2][L_TILE]
  const int64_t d0 = (int64_t)blockIdx.x * LD;
  const int64_t kbeg = (int64_t)blockIdx.y * p.rows_per_part;
  const int64_t kend = min(p.M, kbeg + p.rows_per_part);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  f32x4 acc[RB][2];
#pragma unroll
  for (int i = 0; i < RB; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (int)((kend - kbeg + LK - 1) / LK);
  u32x4 rq[4], rp[4];
  l_g2r(rq, p.Q, p.ldq, d0, p.D, kbeg, kend);
  l_g2r(rp, p.P, p.ldp, 0, p.R, kbeg, kend);
  l_r2s(rq, sQ);
  l_r2s(rp, sP);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) {
      l_g2r(rq, p.Q, p.ldq, d0, p.D, kbeg + (int64_t)(kt + 1) * LK, kend);
      l_g2r(rp, p.P, p.ldp, 0, p.R, kbeg + (int64_t)(kt + 1) * LK, kend);
    }
    const char* q_img = sQ + cur * L_TILE;
    const char* p_img = sP + cur * L_TILE;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 pf[RB], qf[2];
#pragma unroll
      for (int i = 0; i < RB; ++i) pf[i] = l_frag(p_img, i, kk, lane);
#pragma unroll
      for (int j = 0; j < 2; ++j) qf[j] = l_frag(q_img, wave * 2 + j, kk, lane);
#pragma unroll
      for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[j], pf[i], acc[i][j], 0, 0, 0);
    }
    if (more) {
      l_r2s(rq, sQ + (cur ^ 1) * L_TILE);
      l_r2s(rp, sP + (cur ^ 1) * L_TILE);
    }
    __syncthreads();
  }
  // lane owns out row 16 i + (lane & 15), columns d0 + wave*32 + 16 j + 4 (lane >> 4) .. +3 (D % 8 == 0: all or none)
  float* W = p.ws + (int64_t)blockIdx.y * p.R * p.D;
#pragma unroll
  for (int i = 0; i < RB; ++i) {
    const int64_t r = i * 16 + (lane & 15);
    if (r >= p.R) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t d = d0 + wave * 32 + j * 16 + 4 * (lane >> 4);
      if (d < p.D) *reinterpret_cast<f32x4*>(W + r * p.D + d) = acc[i][j];
    }
  }
}

// out = alpha * sum_part ws[part] (+ out), parts in index order; one thread per (row j, 4 columns d)
__global__ void __launch_bounds__(256) lora_wgrad_reduce_kernel(LoraP p) {
  const int64_t groups = p.D / 4;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.R * groups) return;
  const int64_t j = idx / groups, d = (idx - j * groups) * 4;
  const float* W = p.ws + j * p.D + d;
  const int64_t slab = p.R * p.D;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int z = 0; z < p.nparts; ++z) s += *reinterpret_cast<const f32x4*>(W + z * slab);
  if (p.transposed) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      bf16_t* o = p.out + (d + u) * p.ld_out + j;
      float v = p.alpha * s[u];
      if (p.beta) v += bf2f(*o);
      *o = f2bf(v);
    }
  } else {
    bf16_t* o = p.out + j * p.ld_out + d;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float v = p.alpha * s[u];
      if (p.beta) v += bf2f(o[u]);
      o[u] = f2bf(v);
    }
  }
}

// fixed partition of the M rows: enough (slab, part) workgroups for the chip, >= 256 rows per part, 64-row steps
void lora_partition(int64_t M, int64_t D, int64_t& nparts, int64_t& rows_per_part) {
  const int64_t slabs = (D + LD - 1) / LD;
  int64_t n = (L_TARGET_WGS + slabs - 1) / slabs;
  n = n < L_MAX_PARTS ? n : L_MAX_PARTS;
  const int64_t by_rows = (M + 255) / 256;
  n = n < by_rows ? n : by_rows;
  n = n < 1 ? 1 : n;
  rows_per_part = ((M + n - 1) / n + LK - 1) / LK * LK;
  nparts = (M + rows_per_part - 1) / rows_per_part;
}

template <int RB>
int lora_launch(const LoraP& p, int64_t slabs, hipStream_t st) {
  const int smem = 4 * L_TILE;  // 64 KiB
  auto kern = lora_wgrad_kernel<RB>;
  static bool attr_set = false;
  if (!attr_set) {
    hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    attr_set = true;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)slabs, (unsigned)p.nparts), dim3(LT), smem, st, p);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}

}  // namespace

extern "C" int64_t pz_lora_wgrad_ws_bytes(int64_t M, int64_t D, int64_t R) {
  if (M <= 0 || D <= 0 || R <= 0) return 0;
  int64_t nparts, rpp;
  lora_partition(M, D, nparts, rpp);
  return nparts * R * D * 4;
}

extern "C" int pz_lora_wgrad(const void* Q, int64_t ldq, const void* P, int64_t ldp, void* out, int64_t ld_out,
                             int64_t M, int64_t D, int64_t R, int32_t transposed, float alpha, int32_t beta, void* ws,
                             int64_t ws_bytes, void* stream) {
  PZ_CHECK_ARG(Q && P && out && M > 0 && D > 0 && R > 0, "pz_lora_wgrad: bad args");
  PZ_CHECK_ARG(R % 8 == 0 && R <= 128 && D % 8 == 0, "pz_lora_wgrad: R %% 8 == 0, R <= 128, D %% 8 == 0 (R=%lld D=%lld)",
               (long long)R, (long long)D);
  PZ_CHECK_ARG(ldq % 8 == 0 && ldp % 8 == 0 && ldq >= D && ldp >= R && PZ_ALIGNED(Q, 16) && PZ_ALIGNED(P, 16),
               "pz_lora_wgrad: Q / P rows must be 16-byte aligned (ldq / ldp %% 8 == 0)");
  PZ_CHECK_ARG(ld_out >= (transposed ? R : D), "pz_lora_wgrad: ld_out too small");
  PZ_CHECK_ARG(M < (1LL << 31) && D < (1LL << 31), "pz_lora_wgrad: sizes too large");
  int64_t nparts, rpp;
  lora_partition(M, D, nparts, rpp);
  PZ_CHECK_ARG(ws && PZ_ALIGNED(ws, 16) && ws_bytes >= nparts * R * D * 4,
               "pz_lora_wgrad: workspace of %lld bytes needed (pz_lora_wgrad_ws_bytes), 16-byte aligned",
               (long long)(nparts * R * D * 4));
  LoraP p;
  p.Q = (const bf16_t*)Q;
  p.P = (const bf16_t*)P;
  p.out = (bf16_t*)out;
  p.ws = (float*)ws;
  p.ldq = ldq; p.ldp = ldp; p.ld_out = ld_out;
  p.M = M; p.D = D; p.R = R;
  p.rows_per_part = rpp;
  p.nparts = (int)nparts;
  p.transposed = transposed != 0;
  p.beta = beta != 0;
  p.alpha = alpha;
  hipStream_t st = (hipStream_t)stream;
  const int64_t slabs = (D + LD - 1) / LD;
  int rc;
  if (R <= 16) rc = lora_launch<1>(p, slabs, st);
  else if (R <= 32) rc = lora_launch<2>(p, slabs, st);
  else if (R <= 64) rc = lora_launch<4>(p, slabs, st);
  else rc = lora_launch<8>(p, slabs, st);
  if (rc != PZ_OK) return rc;
  const int64_t work = R * (D / 4);
  hipLaunchKernelGGL(lora_wgrad_reduce_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, p);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}
