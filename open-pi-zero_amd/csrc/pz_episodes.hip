// Micro-batch assembly from an episode store in device memory, two launches:
//   pz_episode_gather_frames  uint8 frames [N, C, H, W, 3] at rows idx[B] -> planar uint8 [B * C, 3, H, W]
//   pz_episode_gather_rows    action chunk, proprio history, pad mask, tokens and attention mask of samples idx[B],
//                             clamped at the ends of each sample's own episode
// Both only move bytes (the action / proprio arrays are normalised once, when the store is loaded): no atomics, no
// LDS, every thread writes its own outputs.  Every row read from idx / episode_of is compared with its bound before it
// becomes an address, so a bad index writes and reads nothing.
#include "pz_common.h"

namespace {

constexpr int EP_THREADS = 256;

// selectors of the two v_perm_b32 that pull channel c's four bytes (stream offsets c, c + 3, c + 6, c + 9) out of three
// consecutive dwords A, B, C of interleaved RGB: t = perm(B, A, sel_ab(c)) takes the bytes that lie in A (selector =
// offset, 0..3) or B (selector = offset, 4..7); r = perm(C, t, sel_c(c)) keeps those (selector j) and adds the bytes of
// C (selector 4 + offset - 8)
constexpr unsigned sel_ab(int c) {
  unsigned s = 0;
  for (int j = 0; j < 4; ++j) {
    const int o = c + 3 * j;
    s |= (unsigned)(o < 8 ? o : 0) << (8 * j);
  }
  return s;
}
constexpr unsigned sel_c(int c) {
  unsigned s = 0;
  for (int j = 0; j < 4; ++j) {
    const int o = c + 3 * j;
    s |= (unsigned)(o < 8 ? j : o - 4) << (8 * j);
  }
  return s;
}

template <int CH>
__device__ __forceinline__ unsigned pick4(unsigned a, unsigned b, unsigned c) {
  const unsigned t = __builtin_amdgcn_perm(b, a, sel_ab(CH));
  return __builtin_amdgcn_perm(c, t, sel_c(CH));
}

template <int CH>
__device__ __forceinline__ u32x4 plane16(const u32x4& w0, const u32x4& w1, const u32x4& w2) {
  // the 12 dwords of 16 pixels, in stream order: w0.xyzw, w1.xyzw, w2.xyzw
  return u32x4{pick4<CH>(w0.x, w0.y, w0.z), pick4<CH>(w0.w, w1.x, w1.y), pick4<CH>(w1.z, w1.w, w2.x),
               pick4<CH>(w2.y, w2.z, w2.w)};
}

// one thread per (frame unit, 16-pixel group); a unit is one camera of one sample: out unit u = b * C + cam reads store
// unit idx[b] * C + cam (idx == nullptr: the identity, unit u).  VEC: H * W % 16 == 0 and 16-byte aligned bases, so each
// lane moves 48 contiguous bytes as three 16-byte loads and three 16-byte planar stores; otherwise (and for the last,
// partial group) bytes.
template <bool VEC>
__global__ void __launch_bounds__(EP_THREADS) gather_frames_kernel(
    const uint8_t* __restrict__ store, const int64_t* __restrict__ idx, uint8_t* __restrict__ out, int64_t N,
    int64_t total, int64_t groups, int C, int64_t HW) {
  const int64_t i = (int64_t)blockIdx.x * EP_THREADS + threadIdx.x;
  if (i >= total) return;
  const int64_t u = i / groups, g = i % groups;
  const int64_t b = u / C;
  const int cam = (int)(u % C);
  const int64_t r = idx ? idx[b] : b;
  if (r < 0 || r >= N) return;
  const uint8_t* src = store + ((r * C + cam) * HW + g * 16) * 3;
  uint8_t* dst = out + u * 3 * HW + g * 16;
  if (VEC) {
    const u32x4* s4 = (const u32x4*)src;
    const u32x4 w0 = s4[0], w1 = s4[1], w2 = s4[2];
    *(u32x4*)dst = plane16<0>(w0, w1, w2);
    *(u32x4*)(dst + HW) = plane16<1>(w0, w1, w2);
    *(u32x4*)(dst + 2 * HW) = plane16<2>(w0, w1, w2);
  } else {
    const int n = (int)(HW - g * 16 < 16 ? HW - g * 16 : 16);
    for (int p = 0; p < n; ++p) {
      const uint8_t c0 = src[3 * p], c1 = src[3 * p + 1], c2 = src[3 * p + 2];
      dst[p] = c0;
      dst[HW + p] = c1;
      dst[2 * HW + p] = c2;
    }
  }
}

// one thread per output element of a sample: per = H A + W P + H + L elements, in that order (action, proprio, pad
// mask, token).  Sample b is step t = idx[b] of episode e = episode_of[t], rows [s, en) = offsets[e], offsets[e + 1].
__global__ void __launch_bounds__(EP_THREADS) gather_rows_kernel(
    const float* __restrict__ action, const float* __restrict__ proprio, const int32_t* __restrict__ episode_of,
    const int64_t* __restrict__ offsets, const int32_t* __restrict__ tokens, const int64_t* __restrict__ idx,
    float* __restrict__ o_action, float* __restrict__ o_proprio, uint8_t* __restrict__ o_pad, int64_t* __restrict__ o_ids,
    int64_t* __restrict__ o_att, int64_t total, int64_t N, int64_t E, int A, int P, int L, int W, int H, int32_t pad_id) {
  const int64_t i = (int64_t)blockIdx.x * EP_THREADS + threadIdx.x;
  if (i >= total) return;
  const int nA = H * A, nP = W * P;
  const int per = nA + nP + H + L;
  const int64_t b = i / per;
  int j = (int)(i % per);
  const int64_t t = idx[b];
  if (t < 0 || t >= N) return;
  const int64_t e = episode_of[t];
  if (e < 0 || e >= E) return;
  const int64_t s = offsets[e], en = offsets[e + 1];
  if (s < 0 || en > N || t < s || t >= en) return;
  if (j < nA) {
    const int h = j / A, a = j % A;
    const int64_t row = t + h < en - 1 ? t + h : en - 1;
    o_action[b * nA + j] = action[row * A + a];
    return;
  }
  j -= nA;
  if (j < nP) {
    const int w = j / P, p = j % P;
    const int64_t back = t - W + 1 + w;
    const int64_t row = back > s ? back : s;
    o_proprio[b * nP + j] = proprio[row * P + p];
    return;
  }
  j -= nP;
  if (j < H) {
    o_pad[b * H + j] = t + j <= en - 1 ? 1 : 0;
    return;
  }
  j -= H;
  const int32_t id = tokens[e * L + j];
  o_ids[b * L + j] = id;
  o_att[b * L + j] = id != pad_id ? 1 : 0;
}

inline bool ep_grid(int64_t total, unsigned* blocks) {
  const int64_t nb = (total + EP_THREADS - 1) / EP_THREADS;
  if (nb < 1 || nb > 0x7fffffffll) return false;
  *blocks = (unsigned)nb;
  return true;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int pz_episode_gather_frames(const void* store, int64_t N, int64_t C, int64_t H, int64_t W, const void* idx,
                                        int64_t B, void* out, void* stream) {
  PZ_CHECK_ARG(store && out, "episode_gather_frames: null pointer");
  PZ_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0 && B > 0, "episode_gather_frames: N, C, H, W, B must be positive");
  PZ_CHECK_ARG(H <= PZ_OBS_MAX_EXTENT && W <= PZ_OBS_MAX_EXTENT && C <= 64,
               "episode_gather_frames: H and W are limited to %d, C to 64", PZ_OBS_MAX_EXTENT);
  PZ_CHECK_ARG(idx || B <= N, "episode_gather_frames: identity mode (idx = null) needs B <= N");
  PZ_CHECK_ARG(PZ_ALIGNED(idx, 8), "episode_gather_frames: misaligned idx");
  const int64_t HW = H * W, groups = (HW + 15) / 16;
  PZ_CHECK_ARG(B <= (int64_t)0x7fffffff / C && B * C <= ((int64_t)1 << 40) / groups,
               "episode_gather_frames: too many elements for one launch");
  const int64_t total = B * C * groups;
  unsigned g;
  PZ_CHECK_ARG(ep_grid(total, &g), "episode_gather_frames: too many elements for one launch");
  const bool vec = HW % 16 == 0 && PZ_ALIGNED(store, 16) && PZ_ALIGNED(out, 16);
  if (vec)
    hipLaunchKernelGGL(gather_frames_kernel<true>, dim3(g), dim3(EP_THREADS), 0, ST, (const uint8_t*)store,
                       (const int64_t*)idx, (uint8_t*)out, N, total, groups, (int)C, HW);
  else
    hipLaunchKernelGGL(gather_frames_kernel<false>, dim3(g), dim3(EP_THREADS), 0, ST, (const uint8_t*)store,
                       (const int64_t*)idx, (uint8_t*)out, N, total, groups, (int)C, HW);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}

extern "C" int pz_episode_gather_rows(const void* action, const void* proprio, const void* episode_of,
                                      const void* episode_offsets, const void* tokens, const void* idx, int64_t N,
                                      int64_t E, int64_t A, int64_t P, int64_t L, int64_t B, int64_t W, int64_t H,
                                      int32_t pad_id, void* out_action, void* out_proprio, void* out_pad_mask,
                                      void* out_input_ids, void* out_attention_mask, void* stream) {
  PZ_CHECK_ARG(action && proprio && episode_of && episode_offsets && tokens && idx,
               "episode_gather_rows: null input pointer");
  PZ_CHECK_ARG(out_action && out_proprio && out_pad_mask && out_input_ids && out_attention_mask,
               "episode_gather_rows: null output pointer");
  PZ_CHECK_ARG(N > 0 && E > 0 && E <= N && B > 0, "episode_gather_rows: N, E, B must be positive and E <= N");
  PZ_CHECK_ARG(A > 0 && P > 0 && L > 0 && W > 0 && H > 0 && A <= PZ_OBS_MAX_EXTENT && P <= PZ_OBS_MAX_EXTENT &&
                   L <= PZ_OBS_MAX_EXTENT && W <= PZ_OBS_MAX_EXTENT && H <= PZ_OBS_MAX_EXTENT,
               "episode_gather_rows: A, P, L, W, H must lie in [1, %d]", PZ_OBS_MAX_EXTENT);
  PZ_CHECK_ARG(N <= (int64_t)0x7fffffff && E <= (int64_t)0x7fffffff, "episode_gather_rows: N and E are limited to 2^31 - 1");
  PZ_CHECK_ARG(PZ_ALIGNED(action, 4) && PZ_ALIGNED(proprio, 4) && PZ_ALIGNED(episode_of, 4) && PZ_ALIGNED(tokens, 4) &&
                   PZ_ALIGNED(episode_offsets, 8) && PZ_ALIGNED(idx, 8) && PZ_ALIGNED(out_action, 4) &&
                   PZ_ALIGNED(out_proprio, 4) && PZ_ALIGNED(out_input_ids, 8) && PZ_ALIGNED(out_attention_mask, 8),
               "episode_gather_rows: misaligned pointer");
  const int64_t per = H * A + W * P + H + L;
  PZ_CHECK_ARG(per <= (int64_t)0x7fffffff && B <= ((int64_t)1 << 40) / per,
               "episode_gather_rows: too many elements for one launch");
  unsigned g;
  PZ_CHECK_ARG(ep_grid(B * per, &g), "episode_gather_rows: too many elements for one launch");
  hipLaunchKernelGGL(gather_rows_kernel, dim3(g), dim3(EP_THREADS), 0, ST, (const float*)action, (const float*)proprio,
                     (const int32_t*)episode_of, (const int64_t*)episode_offsets, (const int32_t*)tokens,
                     (const int64_t*)idx, (float*)out_action, (float*)out_proprio, (uint8_t*)out_pad_mask,
                     (int64_t*)out_input_ids, (int64_t*)out_attention_mask, B * per, N, E, (int)A, (int)P, (int)L, (int)W,
                     (int)H, pad_id);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}
