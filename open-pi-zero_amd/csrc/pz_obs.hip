// Observation front end and action back end of the inference path: what the reference spends a host-side
// env adapter on (src/agent/env_adapter/{base,simpler}.py) and its data pipeline's resize (dlimp/utils.py:12-17).
//
//   pz_image_resize_norm   uint8 frames of any size -> bf16 [n, 3, S, S] in the model's pixel normalisation
//   pz_image_resize_u8     the same two passes, storing the rounded uint8 code (input of pz_image_augment)
//   pz_proprio_normalize   raw proprio -> the model's normalised proprio (bound | gaussian statistics)
//   pz_action_denormalize  the model's action chunk -> robot units (trailing dimensions pass through)
//
// The resize is tf.image.resize(method="lanczos3", antialias=True) done separably.  The host builds one tap table per
// axis geometry in fp64 (first index, tap count, weights normalised to sum 1; ops.lanczos3_taps) and keeps it on the
// device as fp32, so no kernel here evaluates a sine.  Two launches: a horizontal pass into a planar fp32 scratch
// [n, 3, H_in, S] (never rounded to uint8 between the passes), then a vertical pass that rounds half-to-even
// (v_rndne_f32 = tf.round), clips to [0, 255] and stores the bf16 value of that code from a 256-entry table the host
// filled with the torch expression of the existing path, ((q / 255 - 0.5) / 0.5).to(bf16) -- so an input already at
// S x S gives the bits that expression gives.
//
// These are gather / elementwise kernels over at most a few hundred thousand elements: one thread per output
// element, consecutive threads on consecutive output columns (the vertical pass reads and writes coalesced rows; the
// horizontal pass's lanes read overlapping windows of one input row, served by L1/L2).  Every table entry is
// bounds-checked against the input extent before it is used as an address, every element is written by exactly one
// lane with an ordinary vector store, and there are no atomics and no cross-workgroup dependencies.
#include "pz_common.h"

namespace {

constexpr int OBS_THREADS = 256;

// taps of output index o on one axis: indices [first, first + cnt) clipped to [0, n_in), weights w[0..cnt)
struct Taps {
  const int* first;
  const int* count;
  const float* w;
  int stride;  // floats per output index in w (<= PZ_OBS_MAX_TAPS)
};

// frames uint8 -> tmp fp32 [n][3][H][S]
template <bool CL>
__global__ void __launch_bounds__(OBS_THREADS) resize_h_kernel(const uint8_t* __restrict__ in, float* __restrict__ tmp,
                                                               int64_t total, int H, int W, int S, Taps t) {
  const int64_t i = (int64_t)blockIdx.x * OBS_THREADS + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % S);
  const int64_t r = i / S;  // (img * 3 + c) * H + y
  const int y = (int)(r % H);
  const int64_t pc = r / H;
  const int c = (int)(pc % 3);
  const int64_t img = pc / 3;
  const int x0 = t.first[ox];
  int cnt = t.count[ox];
  cnt = cnt < t.stride ? cnt : t.stride;
  const float* w = t.w + (int64_t)ox * t.stride;
  // element (img, c, y, x): channels-last ((img*H + y)*W + x)*3 + c, planar ((img*3 + c)*H + y)*W + x
  const uint8_t* row = CL ? in + ((img * H + y) * (int64_t)W) * 3 + c : in + ((img * 3 + c) * (int64_t)H + y) * W;
  float acc = 0.f;
  for (int k = 0; k < cnt; ++k) {
    const int x = x0 + k;
    if ((unsigned)x < (unsigned)W) acc = __builtin_fmaf(w[k], (float)row[CL ? (int64_t)x * 3 : (int64_t)x], acc);
  }
  tmp[i] = acc;
}

// tmp fp32 [n][3][H][S] -> out [n][3][S][S]: OutT = bf16_t stores lut[code], OutT = uint8_t the code itself
// (pz_image_resize_u8: the frame goes on to pz_image_augment)
template <typename OutT>
__global__ void __launch_bounds__(OBS_THREADS) resize_v_kernel(const float* __restrict__ tmp, OutT* __restrict__ out,
                                                               int64_t total, int H, int S, Taps t,
                                                               const bf16_t* __restrict__ lut) {
  const int64_t i = (int64_t)blockIdx.x * OBS_THREADS + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % S);
  const int64_t r = i / S;
  const int oy = (int)(r % S);
  const int64_t pc = r / S;  // img * 3 + c
  const int y0 = t.first[oy];
  int cnt = t.count[oy];
  cnt = cnt < t.stride ? cnt : t.stride;
  const float* w = t.w + (int64_t)oy * t.stride;
  const float* col = tmp + pc * (int64_t)H * S + ox;
  float acc = 0.f;
  for (int k = 0; k < cnt; ++k) {
    const int y = y0 + k;
    if ((unsigned)y < (unsigned)H) acc = __builtin_fmaf(w[k], col[(int64_t)y * S], acc);
  }
  const float q = fminf(fmaxf(__builtin_rintf(acc), 0.f), 255.f);  // half-to-even, then clip; NaN cannot occur
  if constexpr (sizeof(OutT) == 1)
    out[i] = (OutT)q;
  else
    out[i] = lut[(int)q];
}

enum { MODE_BOUND = PZ_OBS_NORM_BOUND, MODE_GAUSSIAN = PZ_OBS_NORM_GAUSSIAN };

// bound: a = lo, b = hi; gaussian: a = mean, b = std.  No FMA contraction: the formulas are evaluated as written.
__global__ void __launch_bounds__(OBS_THREADS) proprio_norm_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                   int64_t total, int D, const float* __restrict__ a,
                                                                   const float* __restrict__ b, int mode) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * OBS_THREADS + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i % D);
  const float v = x[i], p = a[j], q = b[j];
  float o;
  if (mode == MODE_BOUND) {
    o = 2.f * (v - p) / (q - p + 1e-8f) - 1.f;
    o = fminf(fmaxf(o, -1.f), 1.f);
  } else {
    o = (v - p) / (q + 1e-8f);
  }
  y[i] = o;
}

__global__ void __launch_bounds__(OBS_THREADS) action_denorm_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                    int64_t total, int D, int n_pass,
                                                                    const float* __restrict__ a,
                                                                    const float* __restrict__ b, int mode) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * OBS_THREADS + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i % D);
  const float v = x[i];
  float o = v;  // the trailing n_pass dimensions (the gripper) pass through bit for bit
  if (j < D - n_pass) {
    const float p = a[j], q = b[j];
    o = mode == MODE_BOUND ? (v + 1.f) / 2.f * (q - p) + p : v * (q + 1e-8f) + p;
  }
  y[i] = o;
}

// action_denorm_kernel's inverse (robot units -> the model's normalised actions: the committed prefix of DESIGN 7f):
// proprio_norm_kernel's two formulas on the first D - n_pass dimensions, the trailing ones copied
__global__ void __launch_bounds__(OBS_THREADS) action_norm_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                  int64_t total, int D, int n_pass,
                                                                  const float* __restrict__ a,
                                                                  const float* __restrict__ b, int mode) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * OBS_THREADS + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i % D);
  const float v = x[i];
  float o = v;
  if (j < D - n_pass) {
    const float p = a[j], q = b[j];
    if (mode == MODE_BOUND) {
      o = 2.f * (v - p) / (q - p + 1e-8f) - 1.f;
      o = fminf(fmaxf(o, -1.f), 1.f);
    } else {
      o = (v - p) / (q + 1e-8f);
    }
  }
  y[i] = o;
}

// action_denorm_kernel with the committed prefix passed through: rows h < prefix_len[b] of the [B, H, D] output are
// the caller's robot-unit rows `prev`, bit for bit (what the robot executed is what is returned for those steps)
__global__ void __launch_bounds__(OBS_THREADS) action_denorm_prefix_kernel(
    const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ prev,
    const int32_t* __restrict__ pl, int64_t total, int64_t H, int D, int n_pass, const float* __restrict__ a,
    const float* __restrict__ b, int mode) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * OBS_THREADS + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i % D);
  const int64_t r = i / D;
  if ((int64_t)pl[r / H] > r % H) {
    y[i] = prev[i];
    return;
  }
  const float v = x[i];
  float o = v;
  if (j < D - n_pass) {
    const float p = a[j], q = b[j];
    o = mode == MODE_BOUND ? (v + 1.f) / 2.f * (q - p) + p : v * (q + 1e-8f) + p;
  }
  y[i] = o;
}

inline bool obs_grid(int64_t total, unsigned* blocks) {
  const int64_t nb = (total + OBS_THREADS - 1) / OBS_THREADS;
  if (nb < 1 || nb > 0x7fffffffll) return false;
  *blocks = (unsigned)nb;
  return true;
}

inline bool obs_disjoint(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x + (uintptr_t)abytes <= y || y + (uintptr_t)bbytes <= x;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int64_t pz_image_resize_scratch_bytes(int64_t n, int64_t H_in, int64_t S) {
  if (n <= 0 || H_in <= 0 || S <= 0) return 0;
  return n * 3 * H_in * S * (int64_t)sizeof(float);
}

// both resize entry points: code = false stores lut[code] as bf16 (pz_image_resize_norm), true the uint8 code
static int resize_launch(const char* who, bool code, const void* frames, int32_t channels_last, int64_t n, int64_t H_in,
                         int64_t W_in, int64_t S, const void* h_first, const void* h_count, const void* h_w,
                         int64_t h_taps, const void* v_first, const void* v_count, const void* v_w, int64_t v_taps,
                         const void* lut, void* scratch, int64_t scratch_bytes, void* out, void* stream) {
  PZ_CHECK_ARG(frames && out && scratch && (lut || code), "%s: null pointer", who);
  PZ_CHECK_ARG(h_first && h_count && h_w && v_first && v_count && v_w, "%s: null tap table", who);
  PZ_CHECK_ARG(channels_last == 0 || channels_last == 1, "%s: channels_last must be 0 or 1", who);
  PZ_CHECK_ARG(n > 0 && H_in > 0 && W_in > 0 && S > 0, "%s: n, H_in, W_in, S must be positive", who);
  PZ_CHECK_ARG(H_in <= PZ_OBS_MAX_EXTENT && W_in <= PZ_OBS_MAX_EXTENT && S <= PZ_OBS_MAX_EXTENT,
               "%s: H_in, W_in and S are limited to %d", who, PZ_OBS_MAX_EXTENT);
  PZ_CHECK_ARG(h_taps > 0 && v_taps > 0, "%s: tap counts must be positive", who);
  PZ_CHECK_ARG(h_taps <= PZ_OBS_MAX_TAPS && v_taps <= PZ_OBS_MAX_TAPS,
               "%s: %lld x %lld taps per output exceed the limit of %d (PZ_OBS_MAX_TAPS: "
               "a Lanczos-3 downscale of up to %dx)",
               who, (long long)h_taps, (long long)v_taps, PZ_OBS_MAX_TAPS, (PZ_OBS_MAX_TAPS - 2) / 6);
  PZ_CHECK_ARG(PZ_ALIGNED(scratch, 4) && PZ_ALIGNED(out, code ? 1 : 2) && PZ_ALIGNED(lut, 2) &&
                   PZ_ALIGNED(h_w, 4) && PZ_ALIGNED(v_w, 4) && PZ_ALIGNED(h_first, 4) && PZ_ALIGNED(h_count, 4) &&
                   PZ_ALIGNED(v_first, 4) && PZ_ALIGNED(v_count, 4),
               "%s: misaligned pointer", who);
  const int64_t need = pz_image_resize_scratch_bytes(n, H_in, S);
  PZ_CHECK_ARG(scratch_bytes >= need, "%s: scratch has %lld bytes, needs %lld", who, (long long)scratch_bytes,
               (long long)need);
  const int64_t tot_h = n * 3 * H_in * S, tot_v = n * 3 * S * S, osz = code ? 1 : 2;
  const int64_t fbytes = n * 3 * H_in * W_in;
  PZ_CHECK_ARG(obs_disjoint(scratch, need, out, tot_v * osz) && obs_disjoint(scratch, need, frames, fbytes) &&
                   obs_disjoint(out, tot_v * osz, frames, fbytes),
               "%s: frames, scratch and out overlap", who);
  unsigned gh, gv;
  PZ_CHECK_ARG(obs_grid(tot_h, &gh) && obs_grid(tot_v, &gv), "%s: too many elements for one launch", who);
  const Taps th{(const int*)h_first, (const int*)h_count, (const float*)h_w, (int)h_taps};
  const Taps tv{(const int*)v_first, (const int*)v_count, (const float*)v_w, (int)v_taps};
  if (channels_last)
    hipLaunchKernelGGL(resize_h_kernel<true>, dim3(gh), dim3(OBS_THREADS), 0, ST, (const uint8_t*)frames,
                       (float*)scratch, tot_h, (int)H_in, (int)W_in, (int)S, th);
  else
    hipLaunchKernelGGL(resize_h_kernel<false>, dim3(gh), dim3(OBS_THREADS), 0, ST, (const uint8_t*)frames,
                       (float*)scratch, tot_h, (int)H_in, (int)W_in, (int)S, th);
  PZ_CHECK_LAUNCH();
  if (code)
    hipLaunchKernelGGL(resize_v_kernel<uint8_t>, dim3(gv), dim3(OBS_THREADS), 0, ST, (const float*)scratch,
                       (uint8_t*)out, tot_v, (int)H_in, (int)S, tv, (const bf16_t*)lut);
  else
    hipLaunchKernelGGL(resize_v_kernel<bf16_t>, dim3(gv), dim3(OBS_THREADS), 0, ST, (const float*)scratch,
                       (bf16_t*)out, tot_v, (int)H_in, (int)S, tv, (const bf16_t*)lut);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}

extern "C" int pz_image_resize_norm(const void* frames, int32_t channels_last, int64_t n, int64_t H_in, int64_t W_in,
                                    int64_t S, const void* h_first, const void* h_count, const void* h_w,
                                    int64_t h_taps, const void* v_first, const void* v_count, const void* v_w,
                                    int64_t v_taps, const void* lut, void* scratch, int64_t scratch_bytes, void* out,
                                    void* stream) {
  return resize_launch("image_resize_norm", false, frames, channels_last, n, H_in, W_in, S, h_first, h_count, h_w,
                       h_taps, v_first, v_count, v_w, v_taps, lut, scratch, scratch_bytes, out, stream);
}

extern "C" int pz_image_resize_u8(const void* frames, int32_t channels_last, int64_t n, int64_t H_in, int64_t W_in,
                                  int64_t S, const void* h_first, const void* h_count, const void* h_w, int64_t h_taps,
                                  const void* v_first, const void* v_count, const void* v_w, int64_t v_taps,
                                  void* scratch, int64_t scratch_bytes, void* out, void* stream) {
  return resize_launch("image_resize_u8", true, frames, channels_last, n, H_in, W_in, S, h_first, h_count, h_w, h_taps,
                       v_first, v_count, v_w, v_taps, nullptr, scratch, scratch_bytes, out, stream);
}

static int obs_norm_check(const char* who, const void* x, const void* y, int64_t rows, int64_t D, const void* a,
                          const void* b, int32_t mode) {
  PZ_CHECK_ARG(x && y && a && b, "%s: null pointer", who);
  PZ_CHECK_ARG(rows > 0 && D > 0 && D <= PZ_OBS_MAX_EXTENT, "%s: rows and D must be positive (D <= %d)", who,
               PZ_OBS_MAX_EXTENT);
  PZ_CHECK_ARG(mode == MODE_BOUND || mode == MODE_GAUSSIAN, "%s: mode must be PZ_OBS_NORM_BOUND or _GAUSSIAN", who);
  PZ_CHECK_ARG(PZ_ALIGNED(x, 4) && PZ_ALIGNED(y, 4) && PZ_ALIGNED(a, 4) && PZ_ALIGNED(b, 4), "%s: misaligned pointer",
               who);
  return PZ_OK;
}

extern "C" int pz_proprio_normalize(const void* x, void* y, int64_t rows, int64_t D, const void* a, const void* b,
                                    int32_t mode, void* stream) {
  if (int rc = obs_norm_check("proprio_normalize", x, y, rows, D, a, b, mode)) return rc;
  unsigned g;
  PZ_CHECK_ARG(obs_grid(rows * D, &g), "proprio_normalize: too many elements for one launch");
  hipLaunchKernelGGL(proprio_norm_kernel, dim3(g), dim3(OBS_THREADS), 0, ST, (const float*)x, (float*)y, rows * D,
                     (int)D, (const float*)a, (const float*)b, (int)mode);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}

extern "C" int pz_action_denormalize(const void* x, void* y, int64_t rows, int64_t D, int64_t n_pass, const void* a,
                                     const void* b, int32_t mode, void* stream) {
  if (int rc = obs_norm_check("action_denormalize", x, y, rows, D, a, b, mode)) return rc;
  PZ_CHECK_ARG(n_pass >= 0 && n_pass <= D, "action_denormalize: n_pass must be in [0, D]");
  unsigned g;
  PZ_CHECK_ARG(obs_grid(rows * D, &g), "action_denormalize: too many elements for one launch");
  hipLaunchKernelGGL(action_denorm_kernel, dim3(g), dim3(OBS_THREADS), 0, ST, (const float*)x, (float*)y, rows * D,
                     (int)D, (int)n_pass, (const float*)a, (const float*)b, (int)mode);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}

extern "C" int pz_action_normalize(const void* x, void* y, int64_t rows, int64_t D, int64_t n_pass, const void* a,
                                   const void* b, int32_t mode, void* stream) {
  if (int rc = obs_norm_check("action_normalize", x, y, rows, D, a, b, mode)) return rc;
  PZ_CHECK_ARG(n_pass >= 0 && n_pass <= D, "action_normalize: n_pass must be in [0, D]");
  unsigned g;
  PZ_CHECK_ARG(obs_grid(rows * D, &g), "action_normalize: too many elements for one launch");
  hipLaunchKernelGGL(action_norm_kernel, dim3(g), dim3(OBS_THREADS), 0, ST, (const float*)x, (float*)y, rows * D,
                     (int)D, (int)n_pass, (const float*)a, (const float*)b, (int)mode);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}

extern "C" int pz_action_denormalize_prefix(const void* x, void* y, const void* prev, const int32_t* prefix_len,
                                            int64_t B, int64_t H, int64_t D, int64_t n_pass, const void* a,
                                            const void* b, int32_t mode, void* stream) {
  PZ_CHECK_ARG(B > 0 && H > 0, "action_denormalize_prefix: B and H must be positive");
  if (int rc = obs_norm_check("action_denormalize_prefix", x, y, B * H, D, a, b, mode)) return rc;
  PZ_CHECK_ARG(prev && prefix_len && PZ_ALIGNED(prev, 4) && PZ_ALIGNED(prefix_len, 4),
               "action_denormalize_prefix: null or misaligned prev / prefix_len");
  PZ_CHECK_ARG(n_pass >= 0 && n_pass <= D, "action_denormalize_prefix: n_pass must be in [0, D]");
  unsigned g;
  PZ_CHECK_ARG(obs_grid(B * H * D, &g), "action_denormalize_prefix: too many elements for one launch");
  hipLaunchKernelGGL(action_denorm_prefix_kernel, dim3(g), dim3(OBS_THREADS), 0, ST, (const float*)x, (float*)y,
                     (const float*)prev, prefix_len, B * H * D, H, (int)D, (int)n_pass, (const float*)a,
                     (const float*)b, (int)mode);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}
