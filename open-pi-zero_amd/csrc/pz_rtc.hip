// Guidance arithmetic of inference-time real-time chunking (Black et al. 2025): the seed of the
// denoiser's vector-Jacobian product and the guided Euler update.
//
//   pz_rtc_seed    e = w * (target - (action + (1 - t) * v))             fp32 [B, H, A]
//                  dv[b*T + row0 + h, c] = bf16(e[b, h, c]) for c < A; every other element of dv [B*T, 8] is 0
//                  (pad columns, and the proprio rows when the tied group carries them: T = C + H, row0 = C)
//   pz_rtc_euler   g = e + (1 - t) * dA;  action = action + dt * (v + coef[k] * g);  t += dt once per sample
//
// Plain fp32 multiplies and adds in the order written, every one rounded by itself: the file is built with
// -ffp-contract=off, so a numpy float32 restatement (tests/rtc_ref.py) gives the same bits.  w and coef come from
// the host (src/agent/chunking.py): no exp and no division here, and one captured graph serves every delay,
// overlap and beta.  v is addressed as pz_euler_step addresses it (row stride ldv, batch stride v_bstride).
#include "pz_common.h"

namespace {

constexpr int RTC_THREADS = 256;

__global__ void __launch_bounds__(RTC_THREADS) rtc_seed_kernel(const float* __restrict__ action,
                                                              const bf16_t* __restrict__ v, int64_t ldv, int64_t vbs,
                                                              const float* __restrict__ target,
                                                              const float* __restrict__ w, const float* __restrict__ t,
                                                              float* __restrict__ e, bf16_t* __restrict__ dv, int64_t T,
                                                              int64_t row0, int64_t B, int64_t H, int64_t A) {
  const int64_t idx = (int64_t)blockIdx.x * RTC_THREADS + threadIdx.x;
  if (idx >= B * T * 8) return;
  const int64_t r = idx >> 3, c = idx & 7;
  const int64_t b = r / T, h = r % T - row0;
  bf16_t out = 0;
  if (h >= 0 && h < H && c < A) {
    const int64_t i = (b * H + h) * A + c;
    const float x1 = action[i] + (1.f - t[b]) * bf2f(v[b * vbs + h * ldv + c]);
    const float ev = w[b * H + h] * (target[i] - x1);
    e[i] = ev;
    out = f2bf(ev);
  }
  dv[idx] = out;
}

// one workgroup: every element reads t[b] before the barrier, t advances after it
__global__ void __launch_bounds__(RTC_THREADS) rtc_euler_kernel(float* __restrict__ action, const bf16_t* __restrict__ v,
                                                               int64_t ldv, int64_t vbs, const float* __restrict__ e,
                                                               const bf16_t* __restrict__ dA, int64_t ldda,
                                                               float* __restrict__ t, const float* __restrict__ coef,
                                                               int64_t k, int64_t B, int64_t H, int64_t A, float dt) {
  const float ck = coef[k];
  for (int64_t idx = threadIdx.x; idx < B * H * A; idx += RTC_THREADS) {
    const int64_t r = idx / A, c = idx % A;
    const int64_t b = r / H, h = r % H;
    const float g = e[idx] + (1.f - t[b]) * bf2f(dA[r * ldda + c]);
    action[idx] = action[idx] + dt * (bf2f(v[b * vbs + h * ldv + c]) + ck * g);
  }
  __syncthreads();
  for (int64_t b = threadIdx.x; b < B; b += RTC_THREADS) t[b] += dt;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int pz_rtc_seed(const float* action, const void* v, int64_t ldv, int64_t v_bstride, const float* target,
                           const float* w, const float* t, float* e, void* dv, int64_t T, int64_t row0, int64_t B,
                           int64_t H, int64_t A, void* stream) {
  PZ_CHECK_ARG(action && v && target && w && t && e && dv, "rtc_seed: null pointer");
  PZ_CHECK_ARG(B > 0 && H > 0 && A > 0 && A <= 8, "rtc_seed: B, H > 0 and 0 < A <= 8 required");
  PZ_CHECK_ARG(row0 >= 0 && row0 + H <= T, "rtc_seed: action rows [row0, row0 + H) must lie inside the T rows");
  const int64_t n = B * T * 8;
  hipLaunchKernelGGL(rtc_seed_kernel, dim3((unsigned)((n + RTC_THREADS - 1) / RTC_THREADS)), dim3(RTC_THREADS), 0, ST,
                     action, (const bf16_t*)v, ldv, v_bstride, target, w, t, e, (bf16_t*)dv, T, row0, B, H, A);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}

extern "C" int pz_rtc_euler(float* action, const void* v, int64_t ldv, int64_t v_bstride, const float* e,
                            const void* dA, int64_t ldda, float* t, const float* coef, int64_t steps, int64_t k,
                            int64_t B, int64_t H, int64_t A, float dt, void* stream) {
  PZ_CHECK_ARG(action && v && e && dA && t && coef, "rtc_euler: null pointer");
  PZ_CHECK_ARG(B > 0 && H > 0 && A > 0 && ldda >= A, "rtc_euler: B, H, A > 0 and ldda >= A required");
  PZ_CHECK_ARG(k >= 0 && k < steps, "rtc_euler: step index %lld outside the coefficient table [0, %lld)",
               (long long)k, (long long)steps);
  hipLaunchKernelGGL(rtc_euler_kernel, dim3(1), dim3(RTC_THREADS), 0, ST, action, (const bf16_t*)v, ldv, v_bstride, e,
                     (const bf16_t*)dA, ldda, t, coef, k, B, H, A, dt);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}
