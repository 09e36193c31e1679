// Training-image augmentation on the device: the colour jitter and random crop the reference's data
// pipeline applies to every training frame (src/agent/dataset.py:38-70, dlimp/augmentations.py:65-133), as pure
// functions of host-drawn parameters (pizero_native/augment.py) -- no generator runs here.
//
//   pz_image_augment   uint8 frames [n, 3, S, S] | [n, S, S, 3] + fp32 params [n, 8] + int32 mask [n]
//                      -> bf16 [n, 3, S, S] in the model's pixel normalisation (the buffer pz_patchify reads)
//
// One frame of codes q goes through  x = q / 255;  crop (tf.image.crop_and_resize, bilinear, crop size = image size);
// brightness x + d;  contrast (x - m_c) f + m_c, m_c the mean of channel c at that point of the chain;  saturation
// and hue in hexcone HSV;  clip(x, 0, 1) after every op;  q' = min(floor(255.5 x), 255);  out = lut[q'].  The order is
// fixed, the mask picks the subset per frame.
//
// The contrast needs a whole-frame mean in the middle of a per-pixel chain, so there are two launches:
//   pass 1  (skipped when no frame asks for contrast) sums the crop + brightness + clip image per (frame, channel):
//           a frame's pixels are dealt to P = aug_parts(S) workgroups in a fixed interleaved partition, each lane adds
//           its pixels in index order, the workgroup reduces by a fixed shuffle / LDS tree and ONE lane stores the
//           three partial sums to scratch [n][P][3].  No atomics; P depends on S alone, so a frame's sums do not
//           depend on how many frames share the launch, and two runs give the same bits.
//   pass 2  one output pixel per lane, all three channels: sums the frame's P partials in index order (a uniform
//           loop), repeats the gather, applies the chain, stores three bf16 values (consecutive lanes on consecutive
//           columns of each plane).
// The crop's source coordinate is formed in fp64 (two FMAs per pixel): in fp32 its rounding at S = 224 (ulp(223) =
// 1.5e-5 of a pixel, times a code difference of up to 255 between neighbours) alone would be 4e-3 of a code.  All
// else is fp32 with IEEE division.  Every gather index is compared with S before it becomes an address; an index
// outside contributes 0 (crop_and_resize's extrapolation value), which boxes inside [0, 1] never reach.
#include "pz_common.h"

namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_PIX_PER_PART = 4096;  // pass 1: pixels per workgroup before the partition wraps around
constexpr int AUG_MAX_PARTS = 256;

enum {
  OP_CROP = PZ_AUG_CROP,
  OP_BRIGHTNESS = PZ_AUG_BRIGHTNESS,
  OP_CONTRAST = PZ_AUG_CONTRAST,
  OP_SATURATION = PZ_AUG_SATURATION,
  OP_HUE = PZ_AUG_HUE
};

inline int64_t aug_parts(int64_t S) {
  const int64_t p = (S * S + AUG_PIX_PER_PART - 1) / AUG_PIX_PER_PART;
  return p < 1 ? 1 : (p > AUG_MAX_PARTS ? AUG_MAX_PARTS : p);
}

__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// element (c, y, x) of one frame as q / 255; 0 outside the frame
template <bool CL>
__device__ __forceinline__ float texel(const uint8_t* __restrict__ fr, int S, int c, int y, int x) {
  if ((unsigned)y >= (unsigned)S || (unsigned)x >= (unsigned)S) return 0.f;
  const int64_t at = CL ? ((int64_t)y * S + x) * 3 + c : ((int64_t)c * S + y) * S + x;
  return (float)fr[at] / 255.f;
}

struct Box {
  double y0, x0, sy, sx;  // source coordinate of output index i, in pixels: in_y = y0 + i * sy, in_x = x0 + i * sx
};

// tf.image.crop_and_resize with crop size == image size: in = lo (S-1) + i (hi-lo)(S-1)/(S-1); S == 1 samples the
// box centre
__device__ __forceinline__ Box make_box(const float* __restrict__ p, int S) {
  const double e = (double)(S - 1);
  const double y1 = p[0], x1 = p[1], y2 = p[2], x2 = p[3];
  Box b;
  if (S > 1) {
    b.y0 = y1 * e, b.x0 = x1 * e;
    b.sy = (y2 - y1) * e / e, b.sx = (x2 - x1) * e / e;
  } else {
    b.y0 = 0.5 * (y1 + y2) * e, b.x0 = 0.5 * (x1 + x2) * e;
    b.sy = 0.0, b.sx = 0.0;
  }
  return b;
}

// the image after crop + brightness (+ clips) at output pixel (y, x): pass 1 sums it, pass 2 continues from it
template <bool CL>
__device__ __forceinline__ void head_of_chain(const uint8_t* __restrict__ fr, int S, int y, int x, int ops,
                                              const Box& b, float bright, float v[3]) {
  if (ops & OP_CROP) {
    const double in_y = __builtin_fma((double)y, b.sy, b.y0), in_x = __builtin_fma((double)x, b.sx, b.x0);
    const double fy = __builtin_floor(in_y), fx = __builtin_floor(in_x);
    const int top = (int)fy, left = (int)fx;
    const int bot = (int)__builtin_ceil(in_y), right = (int)__builtin_ceil(in_x);
    const float ly = (float)(in_y - fy), lx = (float)(in_x - fx);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float tl = texel<CL>(fr, S, c, top, left), tr = texel<CL>(fr, S, c, top, right);
      const float bl = texel<CL>(fr, S, c, bot, left), br = texel<CL>(fr, S, c, bot, right);
      const float t = tl + (tr - tl) * lx, u = bl + (br - bl) * lx;
      v[c] = clip01(t + (u - t) * ly);
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = texel<CL>(fr, S, c, y, x);
  }
  if (ops & OP_BRIGHTNESS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = clip01(v[c] + bright);
  }
}

// hexcone RGB -> HSV, h in [0, 1)
__device__ __forceinline__ void rgb_to_hsv(const float v[3], float& h, float& s, float& val) {
  const float r = v[0], g = v[1], b = v[2];
  const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
  const float range = mx - mn;
  val = mx;
  s = mx > 0.f ? range / mx : 0.f;
  h = 0.f;
  if (range > 0.f) {
    if (r == mx)
      h = (g - b) / range / 6.f;
    else if (g == mx)
      h = (b - r) / range / 6.f + 2.f / 6.f;
    else
      h = (r - g) / range / 6.f + 4.f / 6.f;
    if (h < 0.f) h += 1.f;
  }
}

__device__ __forceinline__ void hsv_to_rgb(float h, float s, float val, float v[3]) {
  const float dh = h * 6.f;
  const float dr = clip01(fabsf(dh - 3.f) - 1.f);
  const float dg = clip01(2.f - fabsf(dh - 2.f));
  const float db = clip01(2.f - fabsf(dh - 4.f));
  const float oms = 1.f - s;
  v[0] = (oms + s * dr) * val;
  v[1] = (oms + s * dg) * val;
  v[2] = (oms + s * db) * val;
}

// pass 1: part[frame][blockIdx.x][c] = sum over the workgroup's pixels of the head of the chain
template <bool CL>
__global__ void __launch_bounds__(AUG_THREADS)
    augment_sum_kernel(const uint8_t* __restrict__ frames, const float* __restrict__ params,
                       const int* __restrict__ mask, int ops_union, float* __restrict__ part, int S, int P) {
  __shared__ float red[AUG_THREADS / 64];
  const int64_t f = blockIdx.y;
  const int ops = mask[f] & ops_union;
  if (!(ops & OP_CONTRAST)) return;  // uniform over the workgroup: this frame's sums are never read
  const float* p = params + f * 8;
  const uint8_t* fr = frames + f * 3 * (int64_t)S * S;
  const Box b = make_box(p, S);
  const float bright = p[4];
  const int64_t npix = (int64_t)S * S;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int64_t i = (int64_t)blockIdx.x * AUG_THREADS + threadIdx.x; i < npix; i += (int64_t)P * AUG_THREADS) {
    float v[3];
    head_of_chain<CL>(fr, S, (int)(i / S), (int)(i % S), ops, b, bright, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += v[c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float t = block_sum<AUG_THREADS / 64>(acc[c], red);
    if (threadIdx.x == 0) part[(f * P + blockIdx.x) * 3 + c] = t;
  }
}

// pass 2: one output pixel per lane
template <bool CL>
__global__ void __launch_bounds__(AUG_THREADS)
    augment_apply_kernel(const uint8_t* __restrict__ frames, const float* __restrict__ params,
                         const int* __restrict__ mask, int ops_union, const float* __restrict__ part,
                         bf16_t* __restrict__ out, const bf16_t* __restrict__ lut, int S, int P) {
  const int64_t f = blockIdx.y;
  const int ops = mask[f] & ops_union;
  const int64_t npix = (int64_t)S * S;
  const int64_t i = (int64_t)blockIdx.x * AUG_THREADS + threadIdx.x;
  if (i >= npix) return;
  const float* p = params + f * 8;
  const uint8_t* fr = frames + f * 3 * npix;
  const Box b = make_box(p, S);
  float v[3];
  head_of_chain<CL>(fr, S, (int)(i / S), (int)(i % S), ops, b, p[4], v);
  if (ops & OP_CONTRAST) {
    const float factor = p[5];
    float m[3] = {0.f, 0.f, 0.f};
    const float* ps = part + f * P * 3;
    for (int k = 0; k < P; ++k) {
#pragma unroll
      for (int c = 0; c < 3; ++c) m[c] += ps[k * 3 + c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float mean = m[c] / (float)npix;
      v[c] = clip01((v[c] - mean) * factor + mean);
    }
  }
  if (ops & OP_SATURATION) {
    float h, s, val;
    rgb_to_hsv(v, h, s, val);
    hsv_to_rgb(h, clip01(s * p[6]), val, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = clip01(v[c]);
  }
  if (ops & OP_HUE) {
    float h, s, val;
    rgb_to_hsv(v, h, s, val);
    h += p[7];
    h -= __builtin_floorf(h);
    hsv_to_rgb(h, s, val, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = clip01(v[c]);
  }
  bf16_t* o = out + f * 3 * npix + i;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    // convert_image_dtype(saturate=True): floor(255.5 x), at most 255; fmaxf also turns a NaN into code 0
    const int q = (int)fminf(fmaxf(__builtin_floorf(v[c] * 255.5f), 0.f), 255.f);
    o[c * npix] = lut[q];
  }
}

inline bool aug_disjoint(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x + (uintptr_t)abytes <= y || y + (uintptr_t)bbytes <= x;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int64_t pz_image_augment_scratch_bytes(int64_t n, int64_t S) {
  if (n <= 0 || S <= 0 || S > PZ_OBS_MAX_EXTENT) return 0;
  return n * aug_parts(S) * 3 * (int64_t)sizeof(float);
}

extern "C" int pz_image_augment(const void* frames, int32_t channels_last, int64_t n, int64_t S, const void* params,
                                const void* mask, int32_t ops_union, const void* lut, void* scratch,
                                int64_t scratch_bytes, void* out, void* stream) {
  PZ_CHECK_ARG(frames && params && mask && lut && out, "image_augment: null pointer (frames, params, mask, lut, out)");
  PZ_CHECK_ARG(channels_last == 0 || channels_last == 1, "image_augment: channels_last must be 0 or 1");
  PZ_CHECK_ARG(n > 0 && S > 0, "image_augment: n and S must be positive");
  PZ_CHECK_ARG(n <= 65535, "image_augment: n is limited to 65535 frames per call");
  PZ_CHECK_ARG(S <= PZ_OBS_MAX_EXTENT, "image_augment: S is limited to %d", PZ_OBS_MAX_EXTENT);
  PZ_CHECK_ARG((ops_union & ~PZ_AUG_ALL) == 0, "image_augment: ops_union has bits outside PZ_AUG_ALL");
  PZ_CHECK_ARG(PZ_ALIGNED(params, 4) && PZ_ALIGNED(mask, 4), "image_augment: misaligned params or mask pointer");
  PZ_CHECK_ARG(PZ_ALIGNED(out, 2) && PZ_ALIGNED(lut, 2), "image_augment: misaligned out or lut pointer");
  const int64_t fbytes = n * 3 * S * S, obytes = fbytes * 2, pbytes = n * 8 * 4, mbytes = n * 4;
  const int64_t need = pz_image_augment_scratch_bytes(n, S);
  const bool contrast = (ops_union & OP_CONTRAST) != 0;
  if (contrast) {
    PZ_CHECK_ARG(scratch, "image_augment: null scratch with contrast in ops_union");
    PZ_CHECK_ARG(PZ_ALIGNED(scratch, 4), "image_augment: misaligned scratch pointer");
    PZ_CHECK_ARG(scratch_bytes >= need, "image_augment: scratch has %lld bytes, needs %lld", (long long)scratch_bytes,
                 (long long)need);
    PZ_CHECK_ARG(aug_disjoint(scratch, need, out, obytes) && aug_disjoint(scratch, need, frames, fbytes) &&
                     aug_disjoint(scratch, need, params, pbytes) && aug_disjoint(scratch, need, mask, mbytes) &&
                     aug_disjoint(scratch, need, lut, 512),
                 "image_augment: scratch overlaps another buffer");
  }
  PZ_CHECK_ARG(aug_disjoint(out, obytes, frames, fbytes) && aug_disjoint(out, obytes, params, pbytes) &&
                   aug_disjoint(out, obytes, mask, mbytes) && aug_disjoint(out, obytes, lut, 512),
               "image_augment: out overlaps frames, params, mask or lut");
  const int P = (int)aug_parts(S);
  const int64_t bpf = (S * S + AUG_THREADS - 1) / AUG_THREADS;  // <= 2^20 at the extent limit
  const dim3 g1((unsigned)P, (unsigned)n), g2((unsigned)bpf, (unsigned)n), blk(AUG_THREADS);
  const uint8_t* fr = (const uint8_t*)frames;
  const float* pr = (const float*)params;
  const int* mk = (const int*)mask;
  if (contrast) {
    if (channels_last)
      hipLaunchKernelGGL(augment_sum_kernel<true>, g1, blk, 0, ST, fr, pr, mk, (int)ops_union, (float*)scratch,
                         (int)S, P);
    else
      hipLaunchKernelGGL(augment_sum_kernel<false>, g1, blk, 0, ST, fr, pr, mk, (int)ops_union, (float*)scratch,
                         (int)S, P);
    PZ_CHECK_LAUNCH();
  }
  if (channels_last)
    hipLaunchKernelGGL(augment_apply_kernel<true>, g2, blk, 0, ST, fr, pr, mk, (int)ops_union,
                       (const float*)scratch, (bf16_t*)out, (const bf16_t*)lut, (int)S, P);
  else
    hipLaunchKernelGGL(augment_apply_kernel<false>, g2, blk, 0, ST, fr, pr, mk, (int)ops_union,
                       (const float*)scratch, (bf16_t*)out, (const bf16_t*)lut, (int)S, P);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}
