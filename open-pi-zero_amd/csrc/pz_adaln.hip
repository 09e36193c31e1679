// Time-conditioned row passes of the adaLN / adaLN-Zero action expert (vla/modules.py:78-119,
// joint_model.py:70-79,117-126), memory-bound like pz_norm.hip: one wave per row, 16-byte vector loads,
// fp32 statistics.
//   AdaptiveRMSNorm    h  = x * rsqrt(mean(x^2) + eps) * sigmoid(gamma_pre[b] + b_gamma) + beta[b]
//   AdaptiveLayerscale xm = x + y * sigmoid(gate_pre[b] + b_gate)          (the gated residual add)
// The per-sample modulation rows (gamma_pre / beta / gate_pre: cond @ W^T, no bias) are fp32 slices of one
// [B, ldmod] buffer that a single GEMM per forward / denoise step fills; b = row / rows_per_sample.  The
// backward kernels give one workgroup a whole sample, so its per-sample sums are accumulated in a fixed
// order (rows strided over the 4 waves, then the waves folded 0..3): no atomics, bitwise repeatable.
#include "pz_common.h"

namespace {

__device__ __forceinline__ void unpack8(const u32x4& r, float (&v)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(r[i] << 16);
    v[2 * i + 1] = __uint_as_float(r[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ void load8(const bf16_t* p, float (&v)[8]) {
  unpack8(*reinterpret_cast<const u32x4*>(p), v);
}
__device__ __forceinline__ u32x4 pack8(const float (&v)[8]) {
  u32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = pack2bf(v[2 * i], v[2 * i + 1]);
  return r;
}
__device__ __forceinline__ void loadf8(const float* p, float (&v)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = a[i];
    v[4 + i] = b[i];
  }
}
__device__ __forceinline__ void storef8(float* p, const float (&v)[8]) {
  *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
}
__device__ __forceinline__ float sigmoidf_fast(float u) { return fast_rcp(1.f + fast_exp(-u)); }

// sigmoid(pre[b, ch*8 ..] + bias[ch*8 ..]) of one 8-column chunk
__device__ __forceinline__ void sig8(const float* pre, const bf16_t* bias, float (&s)[8]) {
  float p[8], bv[8];
  loadf8(pre, p);
  load8(bias, bv);
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = sigmoidf_fast(p[i] + bv[i]);
}

// ---------------------------------------------------------------- forward ---
// GATE: xm = x + y * sigmoid(gate_pre[b] + gate_b), written out (bf16) and normalised as stored;
// NORM: h = xm * rstd * sigmoid(gamma_pre[b] + gamma_b) + beta[b].  Each row is read once.
template <int MAXC, bool GATE, bool NORM>
__global__ void __launch_bounds__(256) adaln_fwd_kernel(
    const bf16_t* __restrict__ x, int64_t ldx, const bf16_t* __restrict__ y, int64_t ldy,
    const float* __restrict__ gate_pre, const bf16_t* __restrict__ gate_b, bf16_t* xm, int64_t ldxm,
    const float* __restrict__ gamma_pre, const bf16_t* __restrict__ gamma_b, const float* __restrict__ beta,
    bf16_t* h, int64_t ldh, float* rstd, int64_t ldmod, int64_t R, int D, int64_t rps, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int64_t b = row / rps;
  const int nc = D / 8;
  float v[MAXC][8];
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int ch = lane + 64 * c;
    if (ch < nc) {
      load8(x + row * ldx + ch * 8, v[c]);
      if (GATE) {
        float yv[8], s[8];
        load8(y + row * ldy + ch * 8, yv);
        sig8(gate_pre + b * ldmod + ch * 8, gate_b + ch * 8, s);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[c][i] += yv[i] * s[i];
        const u32x4 q = pack8(v[c]);
        *reinterpret_cast<u32x4*>(xm + row * ldxm + ch * 8) = q;
        unpack8(q, v[c]);  // the statistics of the row as stored (what the backward reads)
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) ss += v[c][i] * v[c][i];
    }
  }
  if (!NORM) return;
  // the modulation chunks requested before the row reduction: one memory round trip
  float g[MAXC][8], bt[MAXC][8];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int ch = lane + 64 * c;
    if (ch < nc) {
      sig8(gamma_pre + b * ldmod + ch * 8, gamma_b + ch * 8, g[c]);
      loadf8(beta + b * ldmod + ch * 8, bt[c]);
    }
  }
  ss = warp_sum(ss);
  const float r = rsqrtf(ss / (float)D + eps);
  if (rstd && lane == 0) rstd[row] = r;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int ch = lane + 64 * c;
    if (ch < nc) {
      float o[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = v[c][i] * r * g[c][i] + bt[c][i];
      *reinterpret_cast<u32x4*>(h + row * ldh + ch * 8) = pack8(o);
    }
  }
}

// fold the 4 waves' per-sample accumulators in a fixed order and write the sample's fp32 row
template <int MAXC>
__device__ __forceinline__ void fold_waves(float (*red)[2048], const float (&acc)[MAXC][8], float* out, int D, int lane,
                                           int wave) {
  const int nc = D / 8;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int ch = lane + 64 * c;
    if (ch < nc)
#pragma unroll
      for (int i = 0; i < 8; ++i) red[wave][ch * 8 + i] = acc[c][i];
  }
  __syncthreads();
  for (int n = threadIdx.x; n < D; n += 256) out[n] = ((red[0][n] + red[1][n]) + red[2][n]) + red[3][n];
  __syncthreads();
}

// --------------------------------------------------- adaptive norm backward ---
// one workgroup = one sample (rps rows): dx = dres + d(norm)/dx . dh;
// dgamma_pre[b] = sigma' * sum_rows dh * xhat, dbeta[b] = sum_rows dh
template <int MAXC>
__global__ void __launch_bounds__(256) adaln_norm_bwd_kernel(
    const bf16_t* __restrict__ dh, int64_t lddh, const bf16_t* __restrict__ x, int64_t ldx,
    const float* __restrict__ rstd, const float* __restrict__ gamma_pre, const bf16_t* __restrict__ gamma_b,
    const bf16_t* dres, bf16_t* dx, int64_t lddx, float* dgamma_pre, float* dbeta, int64_t ldmod, int D, int64_t rps) {
  __shared__ float red[4][2048];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = blockIdx.x;
  const int nc = D / 8;
  float g[MAXC][8], dgacc[MAXC][8], dbacc[MAXC][8];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int ch = lane + 64 * c;
#pragma unroll
    for (int i = 0; i < 8; ++i) g[c][i] = dgacc[c][i] = dbacc[c][i] = 0.f;
    if (ch < nc) sig8(gamma_pre + b * ldmod + ch * 8, gamma_b + ch * 8, g[c]);
  }
  for (int64_t rr = wave; rr < rps; rr += 4) {
    const int64_t row = b * rps + rr;
    const float r = rstd[row];
    float xv[MAXC][8], gv[MAXC][8];
    u32x4 dr[MAXC];  // residual gradient: loaded with x / dh, not after the row reduction
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int ch = lane + 64 * c;
      dr[c] = u32x4{0u, 0u, 0u, 0u};
      if (ch < nc && dres) dr[c] = *reinterpret_cast<const u32x4*>(dres + row * lddx + ch * 8);
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int ch = lane + 64 * c;
      if (ch < nc) {
        float dv[8];
        load8(x + row * ldx + ch * 8, xv[c]);
        load8(dh + row * lddh + ch * 8, dv);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          gv[c][i] = dv[i] * g[c][i];
          dot += gv[c][i] * xv[c][i];
          dgacc[c][i] += dv[i] * xv[c][i] * r;
          dbacc[c][i] += dv[i];
        }
      }
    }
    dot = warp_sum(dot);
    const float k = r * r * r * dot / (float)D;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int ch = lane + 64 * c;
      if (ch < nc) {
        float o[8];
        unpack8(dr[c], o);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] += r * gv[c][i] - k * xv[c][i];
        *reinterpret_cast<u32x4*>(dx + row * lddx + ch * 8) = pack8(o);
      }
    }
  }
  if (dgamma_pre) {
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
#pragma unroll
      for (int i = 0; i < 8; ++i) dgacc[c][i] *= g[c][i] * (1.f - g[c][i]);
    fold_waves<MAXC>(red, dgacc, dgamma_pre + b * ldmod, D, lane, wave);
  }
  if (dbeta) fold_waves<MAXC>(red, dbacc, dbeta + b * ldmod, D, lane, wave);
}

// ---------------------------------------------------- gated residual backward ---
// one workgroup = one sample: dy = dout * sigma, dgate_pre[b] = sigma (1 - sigma) * sum_rows dout * y
template <int MAXC>
__global__ void __launch_bounds__(256) adaln_gate_bwd_kernel(
    const bf16_t* __restrict__ dout, int64_t lddo, const bf16_t* __restrict__ y, int64_t ldy,
    const float* __restrict__ gate_pre, const bf16_t* __restrict__ gate_b, bf16_t* dy, int64_t lddy, float* dgate_pre,
    int64_t ldmod, int D, int64_t rps) {
  __shared__ float red[4][2048];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = blockIdx.x;
  const int nc = D / 8;
  float s[MAXC][8], acc[MAXC][8];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int ch = lane + 64 * c;
#pragma unroll
    for (int i = 0; i < 8; ++i) s[c][i] = acc[c][i] = 0.f;
    if (ch < nc) sig8(gate_pre + b * ldmod + ch * 8, gate_b + ch * 8, s[c]);
  }
  for (int64_t rr = wave; rr < rps; rr += 4) {
    const int64_t row = b * rps + rr;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int ch = lane + 64 * c;
      if (ch < nc) {
        float dv[8], yv[8], o[8];
        load8(dout + row * lddo + ch * 8, dv);
        load8(y + row * ldy + ch * 8, yv);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          o[i] = dv[i] * s[c][i];
          acc[c][i] += dv[i] * yv[i];
        }
        *reinterpret_cast<u32x4*>(dy + row * lddy + ch * 8) = pack8(o);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[c][i] *= s[c][i] * (1.f - s[c][i]);
  fold_waves<MAXC>(red, acc, dgate_pre + b * ldmod, D, lane, wave);
}

#define ADALN_DISPATCH(KERNEL, GRID, ...)                                                              \
  do {                                                                                                 \
    const int nc_ = (int)(D / 8);                                                                      \
    if (nc_ <= 64) hipLaunchKernelGGL((KERNEL(1)), GRID, dim3(256), 0, st, __VA_ARGS__);               \
    else if (nc_ <= 128) hipLaunchKernelGGL((KERNEL(2)), GRID, dim3(256), 0, st, __VA_ARGS__);         \
    else if (nc_ <= 192) hipLaunchKernelGGL((KERNEL(3)), GRID, dim3(256), 0, st, __VA_ARGS__);         \
    else hipLaunchKernelGGL((KERNEL(4)), GRID, dim3(256), 0, st, __VA_ARGS__);                         \
  } while (0)

// common argument rules: D, the sample grouping and the fp32 modulation rows
int check_adaln(const char* who, int64_t R, int64_t D, int64_t rps, int64_t ldmod) {
  PZ_CHECK_ARG(D > 0 && D % 8 == 0 && D <= 2048, "%s: D=%lld must be a multiple of 8 and <= 2048", who, (long long)D);
  PZ_CHECK_ARG(R >= 0 && rps > 0 && R % rps == 0, "%s: rows_per_sample=%lld must divide R=%lld", who, (long long)rps,
               (long long)R);
  PZ_CHECK_ARG(ldmod >= D && ldmod % 4 == 0, "%s: ldmod=%lld must be >= D and a multiple of 4", who, (long long)ldmod);
  return PZ_OK;
}
bool rows_ok(const void* p, int64_t ld, int64_t D) { return p && PZ_ALIGNED(p, 16) && ld % 8 == 0 && ld >= D; }
bool mod_ok(const void* p) { return p && PZ_ALIGNED(p, 16); }

}  // namespace

extern "C" int pz_adaln_fwd(const void* x, int64_t ldx, const void* y, int64_t ldy, const float* gate_pre,
                            const void* gate_bias, void* xm, int64_t ldxm, const float* gamma_pre,
                            const void* gamma_bias, const float* beta, void* h, int64_t ldh, float* rstd,
                            int64_t ldmod, int64_t R, int64_t D, int64_t rows_per_sample, float eps, void* stream) {
  int e = check_adaln("adaln_fwd", R, D, rows_per_sample, ldmod);
  if (e) return e;
  const bool gate = y != nullptr, norm = h != nullptr;
  PZ_CHECK_ARG(gate || norm, "adaln_fwd: neither stage requested (y and h are NULL)");
  PZ_CHECK_ARG(rows_ok(x, ldx, D), "adaln_fwd: x rows must be 16-byte aligned");
  if (gate)
    PZ_CHECK_ARG(rows_ok(y, ldy, D) && rows_ok(xm, ldxm, D) && mod_ok(gate_pre) && mod_ok(gate_bias),
                 "adaln_fwd: gate stage needs y, xm (16-byte aligned rows), gate_pre and gate_bias (16-byte aligned)");
  else
    PZ_CHECK_ARG(!xm && !gate_pre, "adaln_fwd: xm / gate_pre given without y");
  if (norm)
    PZ_CHECK_ARG(rows_ok(h, ldh, D) && mod_ok(gamma_pre) && mod_ok(gamma_bias) && mod_ok(beta),
                 "adaln_fwd: norm stage needs h (16-byte aligned rows), gamma_pre, gamma_bias and beta (16-byte aligned)");
  else
    PZ_CHECK_ARG(!rstd && !gamma_pre, "adaln_fwd: rstd / gamma_pre given without h");
  if (R == 0) return PZ_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)((R + 3) / 4));
#define ADALN_FWD_ARGS                                                                                              \
  (const bf16_t*)x, ldx, (const bf16_t*)y, ldy, gate_pre, (const bf16_t*)gate_bias, (bf16_t*)xm, ldxm, gamma_pre,   \
      (const bf16_t*)gamma_bias, beta, (bf16_t*)h, ldh, rstd, ldmod, R, (int)D, rows_per_sample, eps
#define K_GN(C) adaln_fwd_kernel<C, true, true>
#define K_G(C) adaln_fwd_kernel<C, true, false>
#define K_N(C) adaln_fwd_kernel<C, false, true>
  if (gate && norm) ADALN_DISPATCH(K_GN, grid, ADALN_FWD_ARGS);
  else if (gate) ADALN_DISPATCH(K_G, grid, ADALN_FWD_ARGS);
  else ADALN_DISPATCH(K_N, grid, ADALN_FWD_ARGS);
#undef K_GN
#undef K_G
#undef K_N
#undef ADALN_FWD_ARGS
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}

extern "C" int pz_adaln_norm_bwd(const void* dh, int64_t lddh, const void* x, int64_t ldx, const float* rstd,
                                 const float* gamma_pre, const void* gamma_bias, const void* dres, void* dx,
                                 int64_t lddx, float* dgamma_pre, float* dbeta, int64_t ldmod, int64_t R, int64_t D,
                                 int64_t rows_per_sample, void* stream) {
  int e = check_adaln("adaln_norm_bwd", R, D, rows_per_sample, ldmod);
  if (e) return e;
  PZ_CHECK_ARG(rows_ok(dh, lddh, D) && rows_ok(x, ldx, D) && rows_ok(dx, lddx, D) && rstd,
               "adaln_norm_bwd: dh, x, dx rows must be 16-byte aligned and rstd given");
  PZ_CHECK_ARG(!dres || PZ_ALIGNED(dres, 16), "adaln_norm_bwd: dres must be 16-byte aligned");
  PZ_CHECK_ARG(mod_ok(gamma_pre) && mod_ok(gamma_bias) && (!dgamma_pre || mod_ok(dgamma_pre)) &&
                   (!dbeta || mod_ok(dbeta)),
               "adaln_norm_bwd: modulation rows must be 16-byte aligned");
  if (R == 0) return PZ_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)(R / rows_per_sample));
#define K_B(C) adaln_norm_bwd_kernel<C>
  ADALN_DISPATCH(K_B, grid, (const bf16_t*)dh, lddh, (const bf16_t*)x, ldx, rstd, gamma_pre, (const bf16_t*)gamma_bias,
                 (const bf16_t*)dres, (bf16_t*)dx, lddx, dgamma_pre, dbeta, ldmod, (int)D, rows_per_sample);
#undef K_B
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}

extern "C" int pz_adaln_gate_bwd(const void* dout, int64_t lddo, const void* y, int64_t ldy, const float* gate_pre,
                                 const void* gate_bias, void* dy, int64_t lddy, float* dgate_pre, int64_t ldmod,
                                 int64_t R, int64_t D, int64_t rows_per_sample, void* stream) {
  int e = check_adaln("adaln_gate_bwd", R, D, rows_per_sample, ldmod);
  if (e) return e;
  PZ_CHECK_ARG(rows_ok(dout, lddo, D) && rows_ok(y, ldy, D) && rows_ok(dy, lddy, D),
               "adaln_gate_bwd: dout, y, dy rows must be 16-byte aligned");
  PZ_CHECK_ARG(mod_ok(gate_pre) && mod_ok(gate_bias) && mod_ok(dgate_pre),
               "adaln_gate_bwd: gate_pre, gate_bias and dgate_pre must be given, 16-byte aligned");
  if (R == 0) return PZ_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)(R / rows_per_sample));
#define K_Z(C) adaln_gate_bwd_kernel<C>
  ADALN_DISPATCH(K_Z, grid, (const bf16_t*)dout, lddo, (const bf16_t*)y, ldy, gate_pre, (const bf16_t*)gate_bias,
                 (bf16_t*)dy, lddy, dgate_pre, ldmod, (int)D, rows_per_sample);
#undef K_Z
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}
