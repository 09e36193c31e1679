// Training attention of the action expert against a forward-only VLM (train_vlm: False): the T = C + H
// expert tokens of one sample x nh query heads (MQA, head dim 256: every (token, head) is a query row of the same
// keys) against all nk = L keys, of which only rows [key0, key0 + nkeys) -- the expert's own -- carry a gradient.
//
//   pz_expert_attn_fwd   pz_decode_attn's two launches (pz_decode_kernels.h, LSE = true): the same O bits plus the
//                        fp32 log-sum-exp of the capped, masked logits per query row.
//   pz_expert_attn_bwd   expert_attn_bwd_tile: one workgroup per (group of 32-key chunks, sample, 32-row tile), the
//                        forward's decomposition.  Per chunk: S^T = K Q^T and dP^T = V dO^T on the MFMA (K / V
//                        fragments straight from global, Q / dO fragments in registers), p = exp(cap t - lse) and
//                        dS = scale (1 - t^2) p (dP - delta) into LDS as bf16 [row][key] and [key][row], then
//                        dQ^T += K^T dS^T (K staged in a transposed-read LDS image like the forward's V) and, for
//                        chunks that touch the expert's keys, dK^T = Q^T dS and dV^T = dO^T P from the Q / dO images
//                        staged once per workgroup.  fp32 partials go to the workspace: dQ per chunk group, dK / dV
//                        per row tile.  delta = rowsum(dO * O) is computed by the workgroup while it stages dO.
//                        expert_attn_merge_dq / _dkv sum the partials in fixed order and write bf16.
// No atomics: two launches on the same inputs give the same bits.  Keys >= nk are never loaded (sources clamp to
// nk - 1, their p and dS are 0); dK / dV rows outside [key0, key0 + nkeys) are not written.
//
//   pz_expert_attn_fwd_shared / pz_expert_attn_bwd_shared   the same kernels instantiated with SHARED (several flow
//                        draws per observation): the batch counts (observation, draw) pairs, key rows
//                        below prefix come from the observation's K / V (read-only, one copy for all its draws), the
//                        rest from the pair's own compact buffers; dq / dk / dv are written per pair as above.
#include "pz_decode_kernels.h"

namespace {

constexpr int EB_LD = DA_KC + 8;  // bf16 per LDS row of the p / dS tiles (80 B: 16-B aligned rows)

// one 16-B piece of a [32][256] bf16 tile into its transposed-read image (da_vfrag's layout)
__device__ __forceinline__ void eb_stage(char* img, int kr, int ch, u32x4 v) {
  *reinterpret_cast<u32x4*>(img + kr * 512 + (((2 * ch) ^ da_sw(kr)) << 3)) = v;
}

__device__ __forceinline__ float eb_dot8(u32x4 a, u32x4 b) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    s += __uint_as_float(a[i] << 16) * __uint_as_float(b[i] << 16);
    s += __uint_as_float(a[i] & 0xffff0000u) * __uint_as_float(b[i] & 0xffff0000u);
  }
  return s;
}

// workspace: dQ partials [B][ngroups][Rpad][256], then dK and dV partials [B][rtiles][nkeys][256] each (fp32)
struct eb_ws {
  int64_t dq, dk, dv, total;  // float offsets
};
inline eb_ws eb_layout(int64_t B, int64_t rows, int64_t nkeys, int ngroups) {
  const int64_t rtiles = (rows + DA_R - 1) / DA_R, rpad = rtiles * DA_R;
  eb_ws w;
  w.dq = 0;
  w.dk = B * ngroups * rpad * DA_HD;
  w.dv = w.dk + B * rtiles * nkeys * DA_HD;
  w.total = w.dv + B * rtiles * nkeys * DA_HD;
  return w;
}

// grid (ngroups, B * rtiles), 256 threads
template <bool SHARED>
__global__ void __launch_bounds__(256) expert_attn_bwd_tile(pz_expert_attn_bwd_args a, int nch, int64_t ws_dk,
                                                            int64_t ws_dv, da_own_t<SHARED> own) {
  __shared__ __attribute__((aligned(16))) char Kimg[DA_KC * 512];  // one chunk of K
  __shared__ __attribute__((aligned(16))) char Qimg[DA_R * 512];   // the row tile's Q
  __shared__ __attribute__((aligned(16))) char Gimg[DA_R * 512];   // the row tile's dO
  __shared__ __attribute__((aligned(16))) bf16_t dS_s[DA_R][EB_LD];    // dS [row][key]
  __shared__ __attribute__((aligned(16))) bf16_t dST_s[DA_KC][EB_LD];  // dS [key][row]
  __shared__ __attribute__((aligned(16))) bf16_t PT_s[DA_KC][EB_LD];   // p  [key][row]
  __shared__ float lse_s[DA_R], delta_s[DA_R];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int T = (int)a.T, nh = (int)a.nh, nk = (int)a.nk, R = T * nh;
  const int rtiles = (R + DA_R - 1) / DA_R, Rpad = rtiles * DA_R;
  const int grp = blockIdx.x, b = blockIdx.y / rtiles, rt = blockIdx.y % rtiles, r0 = rt * DA_R;
  const bool masked = a.cnt != nullptr;
  const int cnt = masked ? a.cnt[b] : nk;
  int64_t kvb = b;  // batch of the K / V rows (SHARED: the pair's observation)
  const bf16_t *Ko = nullptr, *Vo = nullptr;
  if constexpr (SHARED) {
    kvb = b / (int)own.group;
    Ko = own.k + (int64_t)b * own.bstride;
    Vo = own.v + (int64_t)b * own.bstride;
  }
  const int P = (int)a.prefix;
  const bf16_t* K = (const bf16_t*)a.k + kvb * a.k_bstride;
  const bf16_t* V = (const bf16_t*)a.v + kvb * a.v_bstride;
  const int nchunks = (nk + DA_KC - 1) / DA_KC;
  const int c0 = grp * nch, c1 = min(nchunks, c0 + nch);
  const int key0 = (int)a.key0, key1 = (int)(a.key0 + a.nkeys);
  const int g = lane >> 4;
  // S^T / dP^T tile of this wave: key tile kt (16 keys) x row block rb (16 rows)
  const int kt = wave & 1, rb = wave >> 1;
  const int rl = rb * 16 + (lane & 15), row = r0 + rl;
  const bool rok = row < R;
  const int t = rok ? row / nh : 0, h = rok ? row % nh : 0;
  const int qt = (int)a.qtok0 + t;
  bf16x8 qf[8], gf[8];
  {
    const bf16_t* qp = (const bf16_t*)a.q + ((int64_t)b * a.Lq + a.qoff + t) * a.ldq + (int64_t)h * DA_HD + 8 * g;
    const bf16_t* gp = (const bf16_t*)a.dO + ((int64_t)b * T + t) * a.lddo + (int64_t)h * DA_HD + 8 * g;
#pragma unroll
    for (int dc = 0; dc < 8; ++dc) {
      qf[dc] = rok ? *reinterpret_cast<const bf16x8*>(qp + dc * 32) : bf16x8{};
      gf[dc] = rok ? *reinterpret_cast<const bf16x8*>(gp + dc * 32) : bf16x8{};
    }
  }
  // Q and dO images of the row tile (pad rows zero) and delta = rowsum(dO * O): thread = 4 (row, 16-B piece) pairs,
  // a row's 32 pieces in one half wave
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = threadIdx.x + i * 256, kr = e >> 5, ch = e & 31, rr = r0 + kr;
    const bool ok = rr < R;
    const int tt = ok ? rr / nh : 0, hh = ok ? rr % nh : 0;
    const u32x4 z = {0u, 0u, 0u, 0u};
    const u32x4 qv = ok ? *reinterpret_cast<const u32x4*>((const bf16_t*)a.q + ((int64_t)b * a.Lq + a.qoff + tt) * a.ldq +
                                                          (int64_t)hh * DA_HD + 8 * ch) : z;
    const u32x4 gv = ok ? *reinterpret_cast<const u32x4*>((const bf16_t*)a.dO + ((int64_t)b * T + tt) * a.lddo +
                                                          (int64_t)hh * DA_HD + 8 * ch) : z;
    const u32x4 ov = ok ? *reinterpret_cast<const u32x4*>((const bf16_t*)a.o + ((int64_t)b * T + tt) * a.ldo +
                                                          (int64_t)hh * DA_HD + 8 * ch) : z;
    eb_stage(Qimg, kr, ch, qv);
    eb_stage(Gimg, kr, ch, gv);
    float dl = eb_dot8(gv, ov);
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) dl += __shfl_xor(dl, o, 64);
    if (ch == 0) delta_s[kr] = dl;
  }
  if (threadIdx.x < DA_R) lse_s[threadIdx.x] = r0 + (int)threadIdx.x < R ? a.lse[(int64_t)b * R + r0 + threadIdx.x] : 0.f;
  const float inv_cap = a.cap > 0.f ? 1.f / a.cap : 0.f;
  f32x4 accq[4][2];  // dQ^T tiles: dim tile 4 * wave + i, row tile j (lane: dims 4 (lane >> 4) .. + 3, row lane & 15)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) accq[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  const float my_lse = lse_s[rl], my_delta = delta_s[rl];
  float* wsk = a.ws + ws_dk + ((int64_t)b * rtiles + rt) * a.nkeys * DA_HD;
  float* wsv = a.ws + ws_dv + ((int64_t)b * rtiles + rt) * a.nkeys * DA_HD;
  for (int c = c0; c < c1; ++c) {
    const int j0 = c * DA_KC;
    // K(c) -> LDS image (the previous chunk's reads ended at the loop-closing barrier)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = threadIdx.x + i * 256, kr = e >> 5, ch = e & 31;
      eb_stage(Kimg, kr, ch,
               *reinterpret_cast<const u32x4*>(da_kv_row<SHARED>(K, Ko, min(j0 + kr, nk - 1), P) + 8 * ch));
    }
    {  // S^T and dP^T tiles, then p and dS
      const int key = min(j0 + kt * 16 + (lane & 15), nk - 1);
      const bf16_t* kp = da_kv_row<SHARED>(K, Ko, key, P) + 8 * g;
      const bf16_t* vp = da_kv_row<SHARED>(V, Vo, key, P) + 8 * g;
      f32x4 sv = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int dc = 0; dc < 8; ++dc) {
        sv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(kp + dc * 32), qf[dc], sv, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(vp + dc * 32), gf[dc], dp, 0, 0, 0);
      }
      float ds[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int kl = kt * 16 + 4 * g + e;
        const float x = sv[e] * a.scale;
        float tv = 0.f, lg = x;
        if (a.cap > 0.f) {
          tv = tanh_fast(x * inv_cap);
          lg = a.cap * tv;
        }
        const bool ok = rok && (masked ? da_allowed(qt, j0 + kl, nk, cnt, P, (int)a.cond) : j0 + kl < nk);
        const float p = ok ? __expf(lg - my_lse) : 0.f;
        ds[e] = ok ? a.scale * (1.f - tv * tv) * p * (dp[e] - my_delta) : 0.f;
        dST_s[kl][rl] = f2bf(ds[e]);
        PT_s[kl][rl] = f2bf(p);
      }
      *reinterpret_cast<u32x2*>(&dS_s[rl][kt * 16 + 4 * g]) = u32x2{pack2bf(ds[0], ds[1]), pack2bf(ds[2], ds[3])};
    }
    __syncthreads();
    {  // dQ^T += K^T dS^T
      bf16x8 sb[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) sb[j] = *reinterpret_cast<const bf16x8*>(&dS_s[j * 16 + (lane & 15)][8 * g]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bf16x8 kf = da_vfrag(Kimg, 4 * wave + i, lane);
        accq[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, sb[0], accq[i][0], 0, 0, 0);
        accq[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, sb[1], accq[i][1], 0, 0, 0);
      }
    }
    if (j0 < key1 && j0 + DA_KC > key0) {  // the chunk holds expert keys: dK^T = Q^T dS, dV^T = dO^T P of this row tile
      bf16x8 sb[2], pb[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        sb[j] = *reinterpret_cast<const bf16x8*>(&dST_s[j * 16 + (lane & 15)][8 * g]);
        pb[j] = *reinterpret_cast<const bf16x8*>(&PT_s[j * 16 + (lane & 15)][8 * g]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bf16x8 qi = da_vfrag(Qimg, 4 * wave + i, lane);
        const bf16x8 gi = da_vfrag(Gimg, 4 * wave + i, lane);
        const int d0 = (4 * wave + i) * 16 + 4 * g;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const f32x4 z = {0.f, 0.f, 0.f, 0.f};
          const f32x4 ak = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qi, sb[j], z, 0, 0, 0);
          const f32x4 av = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gi, pb[j], z, 0, 0, 0);
          const int key = j0 + j * 16 + (lane & 15);
          if (key >= key0 && key < key1) {
            *reinterpret_cast<f32x4*>(wsk + (int64_t)(key - key0) * DA_HD + d0) = ak;
            *reinterpret_cast<f32x4*>(wsv + (int64_t)(key - key0) * DA_HD + d0) = av;
          }
        }
      }
    }
    __syncthreads();  // the K image and the p / dS tiles are rewritten by the next chunk
  }
  float* wsq = a.ws + (((int64_t)b * gridDim.x + grp) * Rpad + r0) * DA_HD;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = j * 16 + (lane & 15);
    if (r0 + r >= R) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<f32x4*>(wsq + (int64_t)r * DA_HD + (4 * wave + i) * 16 + 4 * g) = accq[i][j];
  }
}

// grid (R, B), 256 threads: thread = head dim; sums the chunk groups' dQ partials in order 0..ngroups-1
__global__ void __launch_bounds__(256) expert_attn_merge_dq(pz_expert_attn_bwd_args a, int ngroups) {
  const int r = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  const int nh = (int)a.nh, t = r / nh, h = r % nh;
  const int Rpad = ((int)(a.T * a.nh) + DA_R - 1) / DA_R * DA_R;
  const float* ws = a.ws + ((int64_t)b * ngroups * Rpad + r) * DA_HD + d;
  float s = 0.f;
  for (int gI = 0; gI < ngroups; ++gI) s += ws[(int64_t)gI * Rpad * DA_HD];
  ((bf16_t*)a.dq)[((int64_t)b * a.Lq + a.qoff + t) * a.ldq + (int64_t)h * DA_HD + d] = f2bf(s);
}

// grid (nkeys, B, 2), 256 threads: sums the row tiles' dK (z = 0) / dV (z = 1) partials in order 0..rtiles-1
__global__ void __launch_bounds__(256) expert_attn_merge_dkv(pz_expert_attn_bwd_args a, int rtiles, int64_t ws_dk,
                                                             int64_t ws_dv) {
  const int j = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  const bool isv = blockIdx.z == 1;
  const float* ws = a.ws + (isv ? ws_dv : ws_dk) + ((int64_t)b * rtiles * a.nkeys + j) * DA_HD + d;
  float s = 0.f;
  for (int rt = 0; rt < rtiles; ++rt) s += ws[(int64_t)rt * a.nkeys * DA_HD];
  bf16_t* out = isv ? (bf16_t*)a.dv + (int64_t)b * a.dv_bstride : (bf16_t*)a.dk + (int64_t)b * a.dk_bstride;
  out[(int64_t)j * DA_HD + d] = f2bf(s);
}

}  // namespace

extern "C" int64_t pz_expert_attn_bwd_ws_bytes(int64_t B, int64_t rows, int64_t nk, int64_t nkeys) {
  const int nchunks = (int)((nk + DA_KC - 1) / DA_KC);
  int nch, ngroups;
  da_grouping(nchunks, B * ((rows + DA_R - 1) / DA_R), nch, ngroups);
  return eb_layout(B, rows, nkeys, ngroups).total * (int64_t)sizeof(float);
}

namespace {

// argument checks + the three launches of pz_expert_attn_bwd / pz_expert_attn_bwd_shared
template <bool SHARED>
int eb_launch(const pz_expert_attn_bwd_args* a, void* stream, da_own_t<SHARED> own) {
  PZ_CHECK_ARG(a && a->q && a->k && a->v && a->o && a->dO && a->lse && a->dq && a->dk && a->dv && a->ws && a->B > 0 &&
                   a->nh > 0, "expert_attn_bwd: bad args");
  if constexpr (SHARED) {
    const int rc = da_check_own("expert_attn_bwd_shared", own.k, own.v, own.bstride, own.group, a->B, a->nk, a->prefix);
    if (rc != PZ_OK) return rc;
  }
  PZ_CHECK_ARG(a->head_dim == DA_HD && a->T >= 1 && a->T * a->nh <= DA_RMAX && a->nk >= 1,
               "expert_attn_bwd: head_dim 256 and tokens x heads <= 1024 query rows per sample");
  PZ_CHECK_ARG(a->key0 >= 0 && a->nkeys >= 1 && a->key0 + a->nkeys <= a->nk,
               "expert_attn_bwd: the gradient key range [key0, key0 + nkeys) must lie inside [0, nk)");
  PZ_CHECK_ARG(a->qoff >= 0 && a->qoff + a->T <= a->Lq, "expert_attn_bwd: query rows [qoff, qoff + T) outside Lq");
  PZ_CHECK_ARG(a->ws_bytes >= pz_expert_attn_bwd_ws_bytes(a->B, a->T * a->nh, a->nk, a->nkeys),
               "expert_attn_bwd: workspace too small");
  PZ_CHECK_ARG(PZ_ALIGNED(a->q, 16) && PZ_ALIGNED(a->k, 16) && PZ_ALIGNED(a->v, 16) && PZ_ALIGNED(a->o, 16) &&
                   PZ_ALIGNED(a->dO, 16) && PZ_ALIGNED(a->ws, 16) && PZ_ALIGNED(a->lse, 4) && PZ_ALIGNED(a->dq, 2) &&
                   PZ_ALIGNED(a->dk, 2) && PZ_ALIGNED(a->dv, 2) && a->ldq % 8 == 0 && a->ldo % 8 == 0 &&
                   a->lddo % 8 == 0 && a->k_bstride % 8 == 0 && a->v_bstride % 8 == 0,
               "expert_attn_bwd: alignment");
  const int nchunks = (int)((a->nk + DA_KC - 1) / DA_KC);
  const int64_t rows = a->T * a->nh, rtiles = (rows + DA_R - 1) / DA_R;
  PZ_CHECK_ARG(a->B * rtiles < 65536 && a->B < 65536, "expert_attn_bwd: grid too large");
  int nch, ngroups;
  da_grouping(nchunks, a->B * rtiles, nch, ngroups);
  const eb_ws w = eb_layout(a->B, rows, a->nkeys, ngroups);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(expert_attn_bwd_tile<SHARED>, dim3((unsigned)ngroups, (unsigned)(a->B * rtiles)), dim3(256), 0, st,
                     *a, nch, w.dk, w.dv, own);
  PZ_CHECK_LAUNCH();
  hipLaunchKernelGGL(expert_attn_merge_dq, dim3((unsigned)rows, (unsigned)a->B), dim3(256), 0, st, *a, ngroups);
  PZ_CHECK_LAUNCH();
  hipLaunchKernelGGL(expert_attn_merge_dkv, dim3((unsigned)a->nkeys, (unsigned)a->B, 2u), dim3(256), 0, st, *a,
                     (int)rtiles, w.dk, w.dv);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}

}  // namespace

extern "C" int pz_expert_attn_fwd(const pz_decode_attn_args* a, float* lse, void* stream) {
  return da_launch<true>(a, lse, stream);
}

extern "C" int pz_expert_attn_fwd_shared(const pz_decode_attn_args* a, const void* k_own, const void* v_own,
                                         int64_t own_bstride, int64_t kv_group, float* lse, void* stream) {
  return da_launch<true, true>(a, lse, stream, da_own{(const bf16_t*)k_own, (const bf16_t*)v_own, own_bstride, kv_group});
}

extern "C" int pz_expert_attn_bwd(const pz_expert_attn_bwd_args* a, void* stream) {
  return eb_launch<false>(a, stream, da_no_own{});
}

extern "C" int pz_expert_attn_bwd_shared(const pz_expert_attn_bwd_args* a, const void* k_own, const void* v_own,
                                         int64_t own_bstride, int64_t kv_group, void* stream) {
  return eb_launch<true>(a, stream, da_own{(const bf16_t*)k_own, (const bf16_t*)v_own, own_bstride, kv_group});
}
