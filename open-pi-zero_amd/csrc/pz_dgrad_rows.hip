// Input gradient of a Linear for a handful of rows: dx[M, K] = epi(dy[M, N] @ W[N, K]), M <= 16, bf16 in and out,
// fp32 accumulation, W row-major [N, K] as the arena holds it (pz_dgrad_rows; ops.linear_dgrad_rows).
//
// pz_gemm's few-row kernels (GEMV, skinny, skinny-64) all reduce along the contiguous axis of B, so this product
// (B k-strided) lands on the 128-tile kernel: ceil(K / 128) workgroups, each streaming a [N, 128] panel of W.  Here
// the reduction runs along W's ROWS instead, so no transposed copy and no cross-lane traffic is needed:
//   * a lane owns 8 consecutive k columns (one 16-byte load per W row) and keeps acc[M][8] in registers;
//   * the M values dy[:, n] of a row are wave-uniform: a workgroup stages them as fp32 in LDS once per 32 rows of W
//     and every lane reads them as broadcasts;
//   * W goes straight to VGPRs (it is streamed once and shared by nobody): the 8 loads of a wave's rows are issued
//     before the barrier that publishes the dy tile;
//   * a workgroup is 4 waves on one 512-column tile, each on its own rows; their accumulators are summed through LDS
//     in fixed wave order, so N is split 4 ways without 4 slabs;
//   * N is further split over blockIdx.y so that about one workgroup per CU streams; workgroup (kt, s) writes the
//     fp32 partial slab ws[s][M][K] for its columns.
// A second launch sums the S slabs in slab order and applies the epilogue with pz_gemm_epi.h's functor (PZ_EPI_NONE:
// bf16 store; PZ_EPI_DGEGLU: the training backward's derivative from the saved [g | u], in place if dx == aux).
// No atomics, no arrival counters: two stream-ordered launches, bit-identical from run to run whatever the
// workspace and the output held before.
#include "pz_gemm_epi.h"

namespace {

constexpr int DR_THREADS = 256;           // 4 waves
constexpr int DR_WAVES = DR_THREADS / 64;
constexpr int DR_KT = 64 * 8;             // columns per workgroup (8 per lane)
constexpr int DR_U = 8;                   // rows of W per wave and step (16-byte loads in flight per lane)
constexpr int DR_NB = DR_WAVES * DR_U;    // rows of W per workgroup and step
constexpr int DR_RED = DR_WAVES * 4 * DR_KT;  // floats: 4 accumulator rows of every wave

struct DgradRowsP {
  const bf16_t* dy;
  const bf16_t* W;
  float* ws;
  int64_t lddy, ldw;
  int M, N, K, nper;  // nper: rows of W per blockIdx.y
};

template <int MR>  // accumulator rows: M rounded up to 4, 8 or 16
__global__ void __launch_bounds__(DR_THREADS) dgrad_rows_kernel(DgradRowsP p) {
  __shared__ __attribute__((aligned(16))) float sm[DR_RED];  // dy tile [DR_NB][MR] first, then the wave sums
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kt0 = blockIdx.x * DR_KT;
  // lanes past K (K % 8 == 0: whole vectors) load the last vector again and store nothing
  const int kc = min(kt0 + lane * 8, p.K - 8);
  const int n0 = blockIdx.y * p.nper, n1 = min(p.N, n0 + p.nper);

  float acc[MR][8];
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[m][j] = 0.f;

  for (int c0 = n0; c0 < n1; c0 += DR_NB) {
    // rows past n1 re-read row n1 - 1 (in bounds); their dy entries are staged as 0
    u32x4 wv[DR_U];
#pragma unroll
    for (int i = 0; i < DR_U; ++i) {
      const int n = min(c0 + wid * DR_U + i, n1 - 1);
      wv[i] = *reinterpret_cast<const u32x4*>(p.W + (int64_t)n * p.ldw + kc);
    }
    __syncthreads();  // the previous step's reads of the dy tile
    for (int e = tid; e < DR_NB * MR; e += DR_THREADS) {
      const int m = e / DR_NB, nn = e % DR_NB, n = c0 + nn;
      sm[nn * MR + m] = (m < p.M && n < n1) ? bf2f(p.dy[(int64_t)m * p.lddy + n]) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < DR_U; ++i) {
      float w[8];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        w[2 * q] = __uint_as_float(wv[i][q] << 16);
        w[2 * q + 1] = __uint_as_float(wv[i][q] & 0xffff0000u);
      }
      const f32x4* d4 = reinterpret_cast<const f32x4*>(sm + (wid * DR_U + i) * MR);
#pragma unroll
      for (int mq = 0; mq < MR / 4; ++mq) {
        const f32x4 dv = d4[mq];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[mq * 4 + r][j] = __builtin_fmaf(dv[r], w[j], acc[mq * 4 + r][j]);
      }
    }
  }

  // the four waves' accumulators, 4 rows at a time: wave 0 + wave 1 + wave 2 + wave 3, in that order
#pragma unroll
  for (int mg = 0; mg < MR; mg += 4) {
    if (mg >= p.M) break;  // workgroup-uniform
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      f32x4* dst = reinterpret_cast<f32x4*>(sm + (wid * 4 + r) * DR_KT + lane * 8);
      dst[0] = f32x4{acc[mg + r][0], acc[mg + r][1], acc[mg + r][2], acc[mg + r][3]};
      dst[1] = f32x4{acc[mg + r][4], acc[mg + r][5], acc[mg + r][6], acc[mg + r][7]};
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4 * DR_KT / 4 / DR_THREADS; ++i) {
      const int o = tid + DR_THREADS * i;  // 4-column group o of the [4][DR_KT] tile
      const int r = o / (DR_KT / 4), c = (o % (DR_KT / 4)) * 4;
      f32x4 s = *reinterpret_cast<const f32x4*>(sm + r * DR_KT + c);
#pragma unroll
      for (int w = 1; w < DR_WAVES; ++w) s += *reinterpret_cast<const f32x4*>(sm + (w * 4 + r) * DR_KT + c);
      const int m = mg + r, k = kt0 + c;
      if (m < p.M && k < p.K)
        *reinterpret_cast<f32x4*>(p.ws + ((int64_t)blockIdx.y * p.M + m) * p.K + k) = s;
    }
  }
}

// dx = epi(sum_s ws[s]): one lane per (m, 4 columns), slabs added in slab order
template <int EM>
__global__ void __launch_bounds__(64) dgrad_rows_epi_kernel(GemmP p) {
  const int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int64_t kv = p.N >> 2;
  const int64_t m = idx / kv, n = (idx % kv) << 2;
  if (m >= p.M) return;
  const float* src = p.ws + m * p.ldw + n;
  const int64_t slab = p.M * p.ldw;
  f32x4 a = *reinterpret_cast<const f32x4*>(src);
#pragma unroll 8
  for (int64_t s = 1; s < p.ksplit; ++s) a += *reinterpret_cast<const f32x4*>(src + s * slab);
  store_out4_m<EM>(p, 0, 0, m, n, a);
}

struct DrSplit {
  int ktiles, S, nper;
};

// about one workgroup per CU, at least DR_NB rows of W each; nper a multiple of 8
inline DrSplit dr_split(int64_t N, int64_t K) {
  DrSplit d;
  d.ktiles = (int)((K + DR_KT - 1) / DR_KT);
  const int64_t cus = pz_device_cus();
  int64_t S = (cus + d.ktiles - 1) / d.ktiles;
  if (S > N / DR_NB) S = N / DR_NB;
  if (S < 1) S = 1;
  int64_t nper = (N + S - 1) / S;
  nper = (nper + 7) / 8 * 8;
  d.nper = (int)nper;
  d.S = (int)((N + nper - 1) / nper);
  return d;
}

inline bool dr_shape_ok(int64_t M, int64_t N, int64_t K) {
  return M >= 1 && M <= 16 && N >= 8 && K >= 8 && N % 8 == 0 && K % 8 == 0 && N < (1ll << 30) && K < (1ll << 30);
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int64_t pz_dgrad_rows_ws_bytes(int64_t M, int64_t N, int64_t K) {
  if (!dr_shape_ok(M, N, K)) return 0;
  return (int64_t)dr_split(N, K).S * M * K * 4;
}

extern "C" int pz_dgrad_rows(const void* dy, int64_t lddy, const void* W, int64_t ldw, void* dx, int64_t lddx,
                             int64_t M, int64_t N, int64_t K, int32_t epilogue, const void* aux, int64_t ld_aux,
                             void* ws, int64_t ws_bytes, void* stream) {
  PZ_CHECK_ARG(dy && W && dx, "dgrad_rows: null pointer");
  const bool geglu = epilogue == PZ_EPI_DGEGLU;
  const int64_t out_cols = geglu ? 2 * K : K;
  // shapes and layouts the kernel does not take: nothing is launched, the caller runs pz_gemm
  if (!dr_shape_ok(M, N, K) || (epilogue != PZ_EPI_NONE && !geglu) || lddy < N || ldw < K || ldw % 8 != 0 ||
      !PZ_ALIGNED(W, 16) || lddx < out_cols || lddx % 4 != 0 || !PZ_ALIGNED(dx, 8) ||
      (geglu && (!aux || ld_aux < 2 * K || ld_aux % 4 != 0 || !PZ_ALIGNED(aux, 8)))) {
    pz_set_error("dgrad_rows: M=%lld N=%lld K=%lld epilogue=%d (M <= 16, N %% 8 == 0, K %% 8 == 0, PZ_EPI_NONE / "
                 "PZ_EPI_DGEGLU, 16-byte W rows, 8-byte dx / aux rows) is not supported",
                 (long long)M, (long long)N, (long long)K, (int)epilogue);
    return PZ_ERR_UNSUPPORTED;
  }
  const DrSplit sp = dr_split(N, K);
  PZ_CHECK_ARG(ws && PZ_ALIGNED(ws, 16) && ws_bytes >= (int64_t)sp.S * M * K * 4,
               "dgrad_rows: workspace of %lld bytes (16-byte aligned) needed, %lld given",
               (long long)sp.S * M * K * 4, (long long)ws_bytes);
  DgradRowsP p;
  p.dy = (const bf16_t*)dy;
  p.W = (const bf16_t*)W;
  p.ws = (float*)ws;
  p.lddy = lddy;
  p.ldw = ldw;
  p.M = (int)M;
  p.N = (int)N;
  p.K = (int)K;
  p.nper = sp.nper;
  const dim3 grid(sp.ktiles, sp.S);
  if (M <= 4)
    hipLaunchKernelGGL(dgrad_rows_kernel<4>, grid, dim3(DR_THREADS), 0, ST, p);
  else if (M <= 8)
    hipLaunchKernelGGL(dgrad_rows_kernel<8>, grid, dim3(DR_THREADS), 0, ST, p);
  else
    hipLaunchKernelGGL(dgrad_rows_kernel<16>, grid, dim3(DR_THREADS), 0, ST, p);
  PZ_CHECK_LAUNCH();

  GemmP e = {};
  e.C = dx;
  e.ldc = lddx;
  e.M = M;
  e.N = K;  // output columns of the product (DGEGLU writes 2 K)
  e.alpha = 1.f;
  e.epi = epilogue;
  e.aux = (bf16_t*)aux;
  e.ld_aux = ld_aux;
  e.geglu_I = geglu ? K : 0;
  e.ws = (float*)ws;
  e.ksplit = sp.S;
  e.ldw = K;
  const unsigned blocks = (unsigned)((M * (K >> 2) + 63) / 64);
  if (geglu)
    hipLaunchKernelGGL(dgrad_rows_epi_kernel<EM_DGEGLU>, dim3(blocks), dim3(64), 0, ST, e);
  else
    hipLaunchKernelGGL(dgrad_rows_epi_kernel<EM_BF16>, dim3(blocks), dim3(64), 0, ST, e);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}
