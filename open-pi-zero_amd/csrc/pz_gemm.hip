// bf16 MFMA GEMM for gfx950 with fused epilogues (the Pi0 hot-path workhorse).
//
//   C[z](m,n) = epilogue( alpha * sum_k A[z](m,k) * B[z](k,n) )
//
// Operands are bf16 and each may be "k-contiguous" (A stored [M][K], B stored
// [N][K]: nn.Linear weights) or "k-strided" (A stored [K][M], B stored [K][N]).
// That covers forward (NT), dgrad (NN) and wgrad (TN) of every nn.Linear in
// SigLIP / Gemma / the action expert, and the attention products
// S = Q K^T, O = P V, dP = dO V^T, dQ = dS K, dK = dS^T Q, dV = P^T dO
//  without any transpose kernels: k-strided tiles are staged in LDS
// [k][row] and read with ds_read_b64_tr_b16 (gfx950 hardware transpose read).
//
// Tile 128x128x64, 256 threads = 4 waves, mfma_f32_16x16x32_bf16, register
// staged double-buffered LDS (issue-early / write-late, one barrier per K
// step), XOR-swizzled LDS images (conflict-free ds_read_b128 and tr reads),
// XCD-aware tile order.  MFMA operands are swapped (B-frag first) so each lane
// owns 4 consecutive output columns -> vectorised epilogue stores.
#include <type_traits>

#include "pz_gemm_plan.h"

namespace {

constexpr int NT = 256;  // threads of the 128-tile kernel (BM x BN x BK: pz_gemm_plan.h)
constexpr int TILE_BYTES = 128 * 64 * 2;  // one operand tile image in LDS


// two bf16-shaped fragments (8 x 16 bit each = 16 fp8 codes) -> one 32-code f8f6f4 operand
__device__ __forceinline__ i32x8 cat_f8(const bf16x8& lo, const bf16x8& hi) {
  const u32x4 a = __builtin_bit_cast(u32x4, lo), b = __builtin_bit_cast(u32x4, hi);
  return i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
}

__device__ __forceinline__ int sw_tr(int k) { return ((k & 3) | (((k >> 3) & 1) << 2)) << 2; }

// ---- global -> registers (4 x 16 B per thread per operand tile) -------------
template <bool KC>
__device__ __forceinline__ void g2r(u32x4 (&r)[4], const bf16_t* __restrict__ base, int64_t ld,
                                    int64_t row0, int64_t R, int64_t k0, int64_t K,
                                    bool geglu, int64_t gI) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = t + NT * i;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (KC) {
      const int rr = c >> 3, kc = c & 7;
      int64_t grow;
      bool ok;
      if (geglu) {
        const int64_t lr = row0 + (rr & 63);
        ok = lr < gI;
        grow = (rr < 64) ? lr : gI + lr;
      } else {
        grow = row0 + rr;
        ok = grow < R;
      }
      const int64_t kk = k0 + 8 * kc;
      if (ok && kk < K) v = *reinterpret_cast<const u32x4*>(base + grow * ld + kk);
    } else {
      const int kr = c >> 4, rc = c & 15;
      const int64_t kk = k0 + kr, rr = row0 + 8 * rc;
      if (kk < K && rr < R) v = *reinterpret_cast<const u32x4*>(base + kk * ld + rr);
    }
    r[i] = v;
  }
}

template <bool KC>
__device__ __forceinline__ void r2s(const u32x4 (&r)[4], char* lds) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = t + NT * i;
    int off;
    if (KC) {
      const int rr = c >> 3, kc = c & 7;
      off = rr * 128 + ((kc ^ ((rr >> 1) & 7)) << 4);
    } else {
      const int kr = c >> 4, rc = c & 15;
      off = kr * 256 + (((2 * rc) ^ sw_tr(kr)) << 3);
    }
    *reinterpret_cast<u32x4*>(lds + off) = r[i];
  }
}

// fragment for rows rb*16.., k = kk*32 + 8*(lane>>4) + j
template <bool KC, int TRROW = 256>
__device__ __forceinline__ bf16x8 frag(const char* lds, int rb, int kk, int lane) {
  if (KC) {
    const int r = rb * 16 + (lane & 15);
    const int ch = kk * 4 + (lane >> 4);
    return *reinterpret_cast<const bf16x8*>(lds + r * 128 + ((ch ^ ((r >> 1) & 7)) << 4));
  } else {
    const int q = (lane & 15) >> 2, p = lane & 3;
    s16x8 out;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int k = kk * 32 + 8 * (lane >> 4) + 4 * t + q;
      const int off = k * TRROW + (((4 * rb + p) ^ sw_tr(k)) << 3);
      s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4*)(lds + off));
      out[4 * t + 0] = v[0];
      out[4 * t + 1] = v[1];
      out[4 * t + 2] = v[2];
      out[4 * t + 3] = v[3];
    }
    return __builtin_bit_cast(bf16x8, out);
  }
}


// EXT: the rank extension's K-tiles (A2 / B2 / K2) follow the main ones; no split-K, no batch
template <bool AKC, bool BKC, int WM, bool EXT>
__device__ __forceinline__ void gemm_body(const GemmP& p) {
  constexpr int WN = 4 / WM;
  constexpr int MI = (BM / WM) / 16;  // m blocks per wave
  constexpr int NI = (BN / WN) / 16;  // n blocks per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sA = smem;                    // [2][TILE_BYTES]
  char* sB = smem + 2 * TILE_BYTES;   // [2][TILE_BYTES]

  const bool geglu = p.epi == PZ_EPI_GEGLU;
  int tm, tn;
  int64_t z = blockIdx.y;
  if (p.batch_xcd) {
    // workgroups are dealt round-robin over the 8 XCDs: XCD x takes batch entries x, x + 8, ..., each
    // entry's tiles consecutive in its local order (all resident together, sharing the entry's panels)
    const int ntile = p.tiles_m * p.tiles_n, xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
    const int bi = local / ntile, tile = local - bi * ntile;
    z = (int64_t)bi * 8 + xcd;
    tm = tile % p.tiles_m;
    tn = tile / p.tiles_m;
  } else {
    tile_coords(blockIdx.x, gridDim.x, p.tiles_m, p.tiles_n, tm, tn);
  }
  const bool split = p.ksplit > 0;
  const int64_t zo = split ? 0 : z / p.batch_inner, zi = split ? 0 : z % p.batch_inner;
  const bf16_t* A = p.A + zo * p.sAo + zi * p.sAi;
  const bf16_t* B = p.B + zo * p.sBo + zi * p.sBi;
  const int64_t m0 = (int64_t)tm * BM;
  const int64_t n0 = geglu ? (int64_t)tn * (BN / 2) : (int64_t)tn * BN;
  const int64_t kbeg = split ? z * p.ksplit : 0;
  const int64_t kend = split ? min(p.K, kbeg + p.ksplit) : p.K;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / WN, wn = wave % WN;

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk1 = (int)((kend - kbeg + BK - 1) / BK);
  const int nk = EXT ? nk1 + (int)((p.K2 + BK - 1) / BK) : nk1;
  u32x4 ra[4], rb[4];
  auto load = [&](int kt) {
    if (EXT && kt >= nk1) {
      g2r<AKC>(ra, p.A2, p.lda2, m0, p.M, (int64_t)(kt - nk1) * BK, p.K2, false, 0);
      g2r<BKC>(rb, p.B2, p.ldb2, n0, p.N, (int64_t)(kt - nk1) * BK, p.K2, geglu, p.geglu_I);
    } else {
      g2r<AKC>(ra, A, p.lda, m0, p.M, kbeg + (int64_t)kt * BK, kend, false, 0);
      g2r<BKC>(rb, B, p.ldb, n0, p.N, kbeg + (int64_t)kt * BK, kend, geglu, p.geglu_I);
    }
  };
  load(0);
  r2s<AKC>(ra, sA);
  r2s<BKC>(rb, sB);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) load(kt + 1);
    const char* a_img = sA + cur * TILE_BYTES;
    const char* b_img = sB + cur * TILE_BYTES;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[MI], bfr[NI];
#pragma unroll
      for (int i = 0; i < MI; ++i) af[i] = frag<AKC>(a_img, wm * MI + i, kk, lane);
#pragma unroll
      for (int j = 0; j < NI; ++j) bfr[j] = frag<BKC>(b_img, wn * NI + j, kk, lane);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
    }
    if (more) {
      r2s<AKC>(ra, sA + (cur ^ 1) * TILE_BYTES);
      r2s<BKC>(rb, sB + (cur ^ 1) * TILE_BYTES);
    }
    __syncthreads();
  }

  // ---------------------------------------------------------------- epilogue
  if (split) {
    // raw partial sums; GEGLU keeps the [gate | up] column layout of B (cols n, I + n)
    float* W = p.ws + z * p.M * p.ldw;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int64_t m = m0 + wm * (BM / WM) + i * 16 + (lane & 15);
      if (m >= p.M) continue;
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        int64_t n;
        if (geglu) {
          const int64_t nl = n0 + (j % (NI / 2)) * 16 + 4 * (lane >> 4);
          if (nl >= p.geglu_I) continue;
          n = j < NI / 2 ? nl : p.geglu_I + nl;
        } else {
          n = n0 + wn * (BN / WN) + j * 16 + 4 * (lane >> 4);
          if (n >= p.N) continue;
        }
        *reinterpret_cast<f32x4*>(W + m * p.ldw + n) = acc[i][j];
      }
    }
    return;
  }
  const int64_t cofs = zo * p.sCo + zi * p.sCi;
  const int64_t rofs = zo * p.sRo + zi * p.sRi;
  if (geglu) {
    // wave tile = 32 rows x 128 cols: cols [0,64) gate, [64,128) up
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int64_t m = m0 + wm * (BM / WM) + i * 16 + (lane & 15);
#pragma unroll
      for (int j = 0; j < NI / 2; ++j)
        store_geglu4(p, cofs, m, n0 + j * 16 + 4 * (lane >> 4), acc[i][j], acc[i][j + NI / 2]);
    }
    return;
  }
  epi_dispatch(p, [&](auto em) {
    constexpr int EM = decltype(em)::value;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int64_t m = m0 + wm * (BM / WM) + i * 16 + (lane & 15);
#pragma unroll
      for (int j = 0; j < NI; ++j)
        store_out4_m<EM>(p, cofs, rofs, m, n0 + wn * (BN / WN) + j * 16 + 4 * (lane >> 4), acc[i][j]);
    }
  });
}

// TAG only separates kernel symbols (profiling): 1 = the Gemma-2B MLP gate|up GeGLU GEMM (M >= 2048 rows)
template <bool AKC, bool BKC, int WM, int TAG>
__global__ void __launch_bounds__(NT, 2) gemm_kernel(GemmP p) {
  gemm_body<AKC, BKC, WM, false>(p);
}

// ... with the rank extension (pz_gemm_args.K2 > 0)
template <bool AKC, bool BKC, int WM>
__global__ void __launch_bounds__(NT, 2) gemm_x_kernel(GemmP p) {
  gemm_body<AKC, BKC, WM, true>(p);
}

// split-K second pass: C = epilogue(sum_z ws[z]) -- one thread per (row, 4 columns)
__global__ void __launch_bounds__(256) splitk_epilogue_kernel(GemmP p, int S) {
  const bool geglu = p.epi == PZ_EPI_GEGLU;
  const int64_t ncols = geglu ? p.geglu_I : p.N;
  const int64_t groups = (ncols + 3) / 4;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.M * groups) return;
  const int64_t m = idx / groups, n = (idx - m * groups) * 4;
  const float* W = p.ws + m * p.ldw + n;
  const int64_t slab = p.M * p.ldw;
  // slabs loaded 4 at a time (all in flight together), summed in slab order (deterministic)
  auto sum_slabs = [&](const float* src) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int z = 0; z < S; z += 4) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        v[u] = z + u < S ? *reinterpret_cast<const f32x4*>(src + (z + u) * slab) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < 4; ++u) acc += v[u];
    }
    return acc;
  };
  if (geglu) {
    const f32x4 s = sum_slabs(W);
    const f32x4 u = sum_slabs(W + p.geglu_I);
    store_geglu4(p, 0, m, n, s, u);
    return;
  }
  // the epilogue's side inputs (residual, saved activation, bias) issued with the first slabs, not after their sum
  epi_dispatch(p, [&](auto em) {
    constexpr int EM = decltype(em)::value;
    Side sd;
    epi_load4<EM>(p, 0, 0, m, n, sd);
    const u32x2 bias = epi_load_bias(p, n);
    const f32x4 s = sum_slabs(W);
    epi_store4<EM>(p, 0, 0, m, n, s, sd, bias);
  });
}

// 256 x 256 tiles, 512 threads = 8 waves; operands streamed global -> LDS by LDS-DMA (global_load_lds_dwordx4,
// 1 KiB per wave-instruction, no VGPR staging)
// (BT = 256, NT2 = 512: pz_gemm_plan.h)

__device__ __forceinline__ void glds16(const bf16_t* src, char* lds_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_base, 16, 0, 0);
}

#define PZ_WAIT_VM(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")

// -------------------------------------------------------------------------
// 256x256x64 "8-phase" ping-pong GEMM (the dispatched large-GEMM kernel).
//
// 8 waves as 2 (M) x 4 (N), 128 x 64 outputs per wave (acc[8][4], 128 AGPR/VGPR).
// A is k-contiguous (every forward GEMM and the large NN dgrads; a k-strided A takes
// gemm8k_kernel).  Each 64-deep K-tile is consumed in 2 sections of 32 MFMAs: section 0
// reads A-lo + all of B and runs output quadrants (0,0) (0,1), section 1 reads A-hi and
// runs (1,1) (1,0).  Every section = [issue LDS-DMA pieces, ds_reads, counted vmcnt,
// lgkmcnt(0)] barrier [32 MFMA at setprio 1] barrier.  (The older schedule of 4 phases
// of 16 MFMAs measured slower: profiles/r05/feed_ab_*.log.)
// The M-row-1 wave group runs one barrier behind the row-0 group,
// so on every SIMD (waves w and w+4) one wave's MFMAs overlap the other's LDS reads
// / DMA issue.
//
// LDS: two K-tile buffers of 64 KiB, each = 4 regions of 16 KiB:
//   A region 0 (rows with (r % 128) < 64), A region 1 (the other 128 rows),
//   B region 0 (virtual cols 0..127), B region 1 (cols 128..255).
// A region is free as soon as the section (phase) that last reads it has ended,
// so the next-but-one K-tile streams in piece by piece (two sections: A1(kt+1) in
// section 0, A0/B0/B1(kt+2) in section 1); 4 pieces (64 KiB) stay in flight and
// the counted waits (vmcnt 8) never drain the DMA queue in steady state.  Hazards
// (one barrier per section boundary, stagger included): a piece is waited for
// (vmcnt, issuing waves) in a section strictly before the one that reads it; a
// region is restaged >= 1 section after its last read, whose lgkmcnt(0) precedes
// that section's first barrier.
// -------------------------------------------------------------------------
constexpr int P8_BUF = 65536, P8_REG = 16384;

// global row of region-row rr (0..127) of an operand region; B may be the GeGLU [gate; up] stack
template <bool ISA, bool GEGLU>
__device__ __forceinline__ int64_t p8_row(int region, int rr, int64_t row0, int64_t R, int64_t gI) {
  if (ISA) {
    const int64_t g = row0 + (rr >> 6) * 128 + region * 64 + (rr & 63);
    return g < R ? g : R - 1;
  } else if (GEGLU) {
    const int v = region * 128 + rr;  // virtual column: wave (v >> 6), gate/up (v >> 5 & 1)
    int64_t g = row0 + (v >> 6) * 32 + (v & 31);
    g = g < gI ? g : gI - 1;
    return ((v >> 5) & 1) ? gI + g : g;
  } else {
    const int64_t g = row0 + region * 128 + rr;
    return g < R ? g : R - 1;
  }
}

// per-thread global source of DMA instruction i (0/1) of a region image
template <bool KC, bool ISA, bool GEGLU>
__device__ __forceinline__ const bf16_t* p8_src(const bf16_t* base, int64_t ld, int region, int i, int t,
                                                int64_t row0, int64_t R, int64_t gI) {
  if (KC) {  // image [128 rows][64 k], 128-B rows, chunk ch of row r at ch ^ ((r >> 1) & 7)
    const int r = i * 64 + (t >> 3);
    const int ch = (t & 7) ^ ((r >> 1) & 7);
    return base + p8_row<ISA, GEGLU>(region, r, row0, R, gI) * ld + 8 * ch;
  } else {  // whole-operand image [64 k][256 rows], 512-B rows; "region" r = k-rows 32r..32r+31;
            // 16-B chunk c of k-row k at c ^ (sw_tr(k) >> 1) (as the 2-stage kernel's image)
    const int k = region * 32 + i * 16 + (t >> 5);
    const int c = (t & 31) ^ (sw_tr(k) >> 1);
    int64_t g = row0 + 8 * c;  // first of 8 consecutive tile rows
    g = g <= R - 8 ? g : R - 8;
    return base + (int64_t)k * ld + g;
  }
}

// k-strided fragment through inline-asm ds_read_b64_tr_b16.  With the builtin, hipcc cannot
// tell the read from the in-flight LDS-DMA writes and drains the DMA queue (s_waitcnt vmcnt(0))
// before every transposed read, which serialises the 8-phase pipeline.  The asm result is NOT
// tracked by the compiler's lgkmcnt: callers wait lgkmcnt(0) (PZ_WAIT_LGKM0) before any use,
// and a sched_barrier keeps the consuming MFMAs behind that wait.
__device__ __forceinline__ s16x4 ds_tr_asm(const char* p) {
  s16x4 v;
  const unsigned a = (unsigned)(size_t)(const __attribute__((address_space(3))) char*)p;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(a));
  return v;
}

template <int TRROW>
__device__ __forceinline__ bf16x8 frag_tr_asm(const char* lds, int rb, int kk, int lane) {
  const int q = (lane & 15) >> 2, p = lane & 3;
  s16x8 out;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int k = kk * 32 + 8 * (lane >> 4) + 4 * t + q;
    const s16x4 v = ds_tr_asm(lds + k * TRROW + (((4 * rb + p) ^ sw_tr(k)) << 3));
    out[4 * t + 0] = v[0];
    out[4 * t + 1] = v[1];
    out[4 * t + 2] = v[2];
    out[4 * t + 3] = v[3];
  }
  return __builtin_bit_cast(bf16x8, out);
}

#define PZ_SCHED() __builtin_amdgcn_sched_barrier(0)
#define PZ_RAW_BARRIER()           \
  do {                             \
    PZ_SCHED();                    \
    __builtin_amdgcn_s_barrier();  \
    PZ_SCHED();                    \
  } while (0)
#define PZ_WAIT_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

// 8-phase epilogue: wave (wr, wc) owns rows wr*128 + 16*rb + (lane & 15) and columns
// wc*64 + 16*cb + 4*(lane >> 4) .. +3 (GeGLU: gate cb = 0,1 with up cb + 2 of the same column)
// ---- 8-phase epilogue -------------------------------------------------------
// Wave (wr, wc) owns rows wr*128 + 16*rb + (lane & 15) and columns wc*64 + 16*cb + 4*(lane >> 4) .. +3
// (GeGLU: gate cb = 0,1 with up cb + 2 of the same column).  Interior tiles (the vast majority)
// take a lean path per epilogue class: no bounds checks, row pointers stepped by 16 rows, and the
// side inputs (residual / old C / saved activations) of row block rb + 1 loaded before the stores
// of row block rb, so their latency overlaps the stores (vmcnt retires the older loads first).
// Edge tiles use the general per-group store_out4_rt.
enum FastMode { FM_STORE = 0, FM_BF16 = 1, FM_F32 = 2, FM_DACT = 3, FM_DGEGLU = 4 };

__host__ __device__ __forceinline__ int fast_mode(const GemmP& p) {
  if (p.epi == PZ_EPI_DGEGLU) return FM_DGEGLU;
  if (p.epi == PZ_EPI_DGELU || p.epi == PZ_EPI_DSILU) return FM_DACT;
  if (p.c_fp32) return FM_F32;
  if (!p.resid && !p.beta && p.epi == PZ_EPI_NONE) return FM_STORE;
  return FM_BF16;
}

__device__ __forceinline__ u32x2 pk4(const float (&v)[4]) {
  return u32x2{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
}

template <int FM>
__device__ __forceinline__ void epi8p_fast(const GemmP& p, int64_t cofs, int64_t rofs, int64_t m, int64_t nb,
                                           const f32x4 (&acc)[8][4]) {
  const float alpha = p.alpha;
  const int64_t crow = 16 * p.ldc;
  float bias[4][4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    if (FM <= FM_F32 && p.bias) {
      unpack4(*reinterpret_cast<const u32x2*>(p.bias + nb + cb * 16), bias[cb]);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) bias[cb][r] = 0.f;
    }
  }
  if constexpr (FM == FM_STORE) {
    bf16_t* C = reinterpret_cast<bf16_t*>(p.C) + cofs + m * p.ldc + nb;
#pragma unroll
    for (int rb = 0; rb < 8; ++rb) {
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc[rb][cb][r] * alpha + bias[cb][r];
        *reinterpret_cast<u32x2*>(C + rb * crow + cb * 16) = pk4(v);
      }
    }
  } else if constexpr (FM == FM_F32) {
    float* C = reinterpret_cast<float*>(p.C) + cofs + m * p.ldc + nb;
    const bf16_t* R = p.resid ? p.resid + rofs + m * p.ld_resid + nb : nullptr;
    const int64_t rrow = 16 * p.ld_resid;
    const bool ld = p.beta || R;
    f32x4 side[2][4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      side[0][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
      side[1][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    auto load = [&](int rb, f32x4 (&d)[4]) {
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        if (p.beta) {
          d[cb] = *reinterpret_cast<const f32x4*>(C + rb * crow + cb * 16);
        } else {
          float x[4];
          unpack4(*reinterpret_cast<const u32x2*>(R + rb * rrow + cb * 16), x);
          d[cb] = f32x4{x[0], x[1], x[2], x[3]};
        }
      }
    };
    if (ld) load(0, side[0]);
#pragma unroll
    for (int rb = 0; rb < 8; ++rb) {
      if (ld && rb + 1 < 8) load(rb + 1, side[(rb + 1) & 1]);
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc[rb][cb][r] * alpha + bias[cb][r] + side[rb & 1][cb][r];
        *reinterpret_cast<f32x4*>(C + rb * crow + cb * 16) = v;
      }
    }
  } else {
    // bf16 output with side inputs: FM_BF16 (resid and/or old C, optional GELU/SILU with saved
    // pre-activation), FM_DACT (aux = pre-activation), FM_DGEGLU (aux = [g | u], two outputs)
    bf16_t* C = reinterpret_cast<bf16_t*>(p.C) + cofs + m * p.ldc + nb;
    const bool aux_in = FM == FM_DACT || FM == FM_DGEGLU;
    const bf16_t* X0 = aux_in ? p.aux + m * p.ld_aux + nb : (p.beta ? C : nullptr);
    const int64_t x0row = aux_in ? 16 * p.ld_aux : crow;
    const bf16_t* X1 = FM == FM_DGEGLU ? X0 + p.geglu_I : (FM == FM_BF16 && p.resid ? p.resid + rofs + m * p.ld_resid + nb : nullptr);
    const int64_t x1row = FM == FM_DGEGLU ? x0row : 16 * p.ld_resid;
    u32x2 s0[2][4], s1[2][4];
    auto load = [&](int rb, u32x2 (&d0)[4], u32x2 (&d1)[4]) {
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        d0[cb] = X0 ? *reinterpret_cast<const u32x2*>(X0 + rb * x0row + cb * 16) : u32x2{0u, 0u};
        d1[cb] = X1 ? *reinterpret_cast<const u32x2*>(X1 + rb * x1row + cb * 16) : u32x2{0u, 0u};
      }
    };
    load(0, s0[0], s1[0]);
    const bool act = FM == FM_BF16 && (p.epi == PZ_EPI_GELU || p.epi == PZ_EPI_SILU);
    const bool gelu = p.epi == PZ_EPI_GELU || p.epi == PZ_EPI_DGELU;
    bf16_t* Aux = act && p.aux ? p.aux + m * p.ld_aux + nb : nullptr;
    const int64_t arow = 16 * p.ld_aux;
#pragma unroll
    for (int rb = 0; rb < 8; ++rb) {
      if (rb + 1 < 8) load(rb + 1, s0[(rb + 1) & 1], s1[(rb + 1) & 1]);
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        float v[4], x0[4], x1[4];
        unpack4(s0[rb & 1][cb], x0);
        unpack4(s1[rb & 1][cb], x1);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc[rb][cb][r] * alpha;
        bf16_t* Cp = C + rb * crow + cb * 16;
        if constexpr (FM == FM_DGEGLU) {
          float dg[4], du[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float gl_, gr_;
            gelu_tanh_both(x0[r], gl_, gr_);
            dg[r] = v[r] * x1[r] * gr_;
            du[r] = v[r] * gl_;
          }
          *reinterpret_cast<u32x2*>(Cp) = pk4(dg);
          *reinterpret_cast<u32x2*>(Cp + p.geglu_I) = pk4(du);
        } else if constexpr (FM == FM_DACT) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] *= gelu ? gelu_tanh_grad(x0[r]) : silu_grad(x0[r]);
          *reinterpret_cast<u32x2*>(Cp) = pk4(v);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += bias[cb][r];
          if (act) {
            if (Aux) *reinterpret_cast<u32x2*>(Aux + rb * arow + cb * 16) = pk4(v);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = gelu ? gelu_tanh(v[r]) : silu(v[r]);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += x1[r] + x0[r];  // resid, old C (zeros when absent)
          *reinterpret_cast<u32x2*>(Cp) = pk4(v);
        }
      }
    }
  }
}

// ---- LDS-staged output images (interior tiles) ------------------------------------------------
// A swapped-operand MFMA accumulator gives each lane 4 consecutive columns of one row, so direct
// stores are 8 B per lane spread over 16 rows (32-B pieces of many cache lines per instruction).
// Plain and GeGLU interior tiles instead write bf16 256 x 128 images into the idle LDS (16-B chunk
// index XOR-swizzled by row: conflict-free 8-B writes and 16-B reads) and copy them out row-
// contiguously, 16 B per lane (each wave instruction = 4 full 256-B row segments).
__device__ __forceinline__ void img_put(char* img, int row, int col, u32x2 v) {
  const int ch = col >> 3;
  *reinterpret_cast<u32x2*>(img + row * 256 + ((ch ^ (row & 15)) << 4) + ((col >> 2) & 1) * 8) = v;
}
// 16-B output store (non-temporal stores measured no faster for C or the saved activations: profiles/r03/bench_ntaux.json)
__device__ __forceinline__ void st16(bf16_t* dst, const u32x4& v) { *reinterpret_cast<u32x4*>(dst) = v; }
__device__ __forceinline__ void img_flush(const char* img, bf16_t* dst, int64_t ld) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = threadIdx.x + i * NT2, row = c >> 4, ch = c & 15;
    const u32x4 v = *reinterpret_cast<const u32x4*>(img + row * 256 + ((ch ^ (row & 15)) << 4));
    st16(dst + row * ld + ch * 8, v);
  }
}
__device__ __forceinline__ void lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// staged epilogue with side inputs (interior tiles): alpha*acc (+bias) -> two bf16 256 x 128 LDS images,
// then each thread finishes 16-B row chunks: residual / old C / saved activations are read as 16-B
// row-contiguous loads (a batch of 8 chunks in flight), outputs written as 16-B stores.
//   FM_BF16: [aux = pre; act(pre)] (+ resid) (+ old C);  FM_DACT: * act'(aux);  FM_DGEGLU: d(gate|up)
__device__ __forceinline__ void unpack8(const u32x4& w, float (&o)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[2 * i] = __uint_as_float(w[i] << 16);
    o[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ u32x4 pack8v(const float (&v)[8]) {
  return u32x4{pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
}

template <int FM>
__device__ __forceinline__ void epi8p_staged(const GemmP& p, int64_t cofs, int64_t rofs, int64_t m0, int64_t n0,
                                             int wr, int wc, int lane, const f32x4 (&acc)[8][4], char* smem) {
  const int g4 = 4 * (lane >> 4), rl = lane & 15;
  const int64_t nb = n0 + wc * 64 + g4;
  char* img = smem + (wc >> 1) * 65536;
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    float bias[4] = {0.f, 0.f, 0.f, 0.f};
    if (FM == FM_BF16 && p.bias) unpack4(*reinterpret_cast<const u32x2*>(p.bias + nb + cb * 16), bias);
#pragma unroll
    for (int rb = 0; rb < 8; ++rb) {
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[rb][cb][r] * p.alpha + bias[r];
      img_put(img, wr * 128 + rb * 16 + rl, (wc & 1) * 64 + cb * 16 + g4, u32x2{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])});
    }
  }
  lds_sync();
  bf16_t* C = reinterpret_cast<bf16_t*>(p.C) + cofs + m0 * p.ldc + n0;
  const bf16_t* X0 = nullptr;  // side input 0: aux (DACT: pre-activation, DGEGLU: g) or old C
  const bf16_t* X1 = nullptr;  // side input 1: resid or DGEGLU u
  int64_t ld0 = 0, ld1 = 0;
  if (FM == FM_DACT || FM == FM_DGEGLU) {
    X0 = p.aux + m0 * p.ld_aux + n0;
    ld0 = p.ld_aux;
    if (FM == FM_DGEGLU) {
      X1 = X0 + p.geglu_I;
      ld1 = p.ld_aux;
    }
  } else {
    if (p.beta) {
      X0 = C;
      ld0 = p.ldc;
    }
    if (p.resid) {
      X1 = p.resid + rofs + m0 * p.ld_resid + n0;
      ld1 = p.ld_resid;
    }
  }
  const bool act = FM == FM_BF16 && (p.epi == PZ_EPI_GELU || p.epi == PZ_EPI_SILU);
  const bool gelu = p.epi == PZ_EPI_GELU || p.epi == PZ_EPI_DGELU;
  // side inputs in 4 batches of 4 chunks (8 x 16 B per thread in flight); batches of 8 chunks (128 KiB per CU in
  // flight) make hipcc spill 136-172 B in every non-GeGLU 8-phase kernel, so they were not measured
  constexpr int CPB = 4;
#pragma unroll
  for (int half = 0; half < 16 / CPB; ++half) {  // a batch's loads issued together
    u32x4 a0[CPB], a1[CPB], iv[CPB];
#pragma unroll
    for (int i = 0; i < CPB; ++i) {
      const int c = threadIdx.x + (half * CPB + i) * NT2;  // 0 .. 8191 over the two images
      const int im = c >> 12, row = (c >> 4) & 255, ch = c & 15;
      const int col = im * 128 + ch * 8;
      iv[i] = *reinterpret_cast<const u32x4*>(smem + im * 65536 + row * 256 + ((ch ^ (row & 15)) << 4));
      a0[i] = X0 ? *reinterpret_cast<const u32x4*>(X0 + row * ld0 + col) : u32x4{0u, 0u, 0u, 0u};
      a1[i] = X1 ? *reinterpret_cast<const u32x4*>(X1 + row * ld1 + col) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int i = 0; i < CPB; ++i) {
      const int c = threadIdx.x + (half * CPB + i) * NT2;
      const int im = c >> 12, row = (c >> 4) & 255, ch = c & 15;
      const int col = im * 128 + ch * 8;
      float v[8], x0[8], x1[8];
      unpack8(iv[i], v);
      unpack8(a0[i], x0);
      unpack8(a1[i], x1);
      bf16_t* Cp = C + row * p.ldc + col;
      if (FM == FM_DGEGLU) {
        float dg[8], du[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float gl_, gr_;
          gelu_tanh_both(x0[e], gl_, gr_);
          dg[e] = v[e] * x1[e] * gr_;
          du[e] = v[e] * gl_;
        }
        st16(Cp, pack8v(dg));
        st16(Cp + p.geglu_I, pack8v(du));
      } else if (FM == FM_DACT) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= gelu ? gelu_tanh_grad(x0[e]) : silu_grad(x0[e]);
        st16(Cp, pack8v(v));
      } else {
        if (act) {
          if (p.aux) st16(p.aux + (m0 + row) * p.ld_aux + n0 + col, iv[i]);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = gelu ? gelu_tanh(v[e]) : silu(v[e]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += x1[e] + x0[e];  // resid, old C (zeros when absent)
        st16(Cp, pack8v(v));
      }
    }
  }
}

// fused RoPE + Q / K / V scatter (pz_gemm_qkv_rope): the tile (256 rows x one head of 256 columns) is
// rounded to bf16 into two LDS images (columns 0..127 | 128..255 = the two halves of every rotation pair,
// utils.py:4-16 rotate_half), then each thread rotates 16-B chunk pairs (i..i+7 with i+128..i+135) and
// writes them to the joint buffers -- the arithmetic of qkv_rope_split_kernel on the same bf16 inputs.
__device__ __forceinline__ void epi8p_rope(const GemmP& p, int64_t m0, int64_t n0, int wr, int wc, int lane,
                                           const f32x4 (&acc)[8][4], char* smem) {
  const int g4 = 4 * (lane >> 4), rl = lane & 15;
  char* img = smem + (wc >> 1) * 65536;
#pragma unroll
  for (int rb = 0; rb < 8; ++rb)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[rb][cb][r] * p.alpha;
      img_put(img, wr * 128 + rb * 16 + rl, (wc & 1) * 64 + cb * 16 + g4, u32x2{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])});
    }
  lds_sync();
  const int64_t h = n0 >> 8;  // head: 0..nh-1 query, nh key, nh+1 value
#pragma unroll 2
  for (int it = 0; it < 8; ++it) {
    const int c = threadIdx.x + it * NT2, row = c >> 4, ch = c & 15;
    const int64_t m = m0 + row;
    if (m >= p.M) continue;
    const int off = (ch ^ (row & 15)) << 4;
    const u32x4 w1 = *reinterpret_cast<const u32x4*>(smem + row * 256 + off);
    const u32x4 w2 = *reinterpret_cast<const u32x4*>(smem + 65536 + row * 256 + off);
    const int64_t b = m / p.rT, t = m - b * p.rT;
    if (h == p.rnh + 1) {  // value head: copied
      bf16_t* dv = p.rv + (b * p.rLk + p.rkoff + t) * 256 + ch * 8;
      *reinterpret_cast<u32x4*>(dv) = w1;
      *reinterpret_cast<u32x4*>(dv + 128) = w2;
      continue;
    }
    float x1[8], x2[8], o1[8], o2[8];
    unpack8(w1, x1);
    unpack8(w2, x2);
    const float4* cs = reinterpret_cast<const float4*>(p.rcs + p.rpos[m] * 256 + 16 * ch);  // (cos, sin) x 8
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 c2 = cs[q];
      const float co0 = c2.x, si0 = c2.y, co1 = c2.z, si1 = c2.w;
      rope_pair(x1[2 * q], x2[2 * q], co0, si0, o1[2 * q], o2[2 * q]);
      rope_pair(x1[2 * q + 1], x2[2 * q + 1], co1, si1, o1[2 * q + 1], o2[2 * q + 1]);
    }
    bf16_t* d = h < p.rnh ? p.rq + (b * p.rLq + p.rqoff + t) * (p.rnh * 256) + h * 256 + ch * 8
                          : p.rk + (b * p.rLk + p.rkoff + t) * 256 + ch * 8;
    *reinterpret_cast<u32x4*>(d) = pack8v(o1);
    *reinterpret_cast<u32x4*>(d + 128) = pack8v(o2);
  }
}

template <bool GEGLU>
__device__ __forceinline__ void epilogue8p(const GemmP& p, int64_t cofs, int64_t rofs, int64_t m0, int64_t n0,
                                           int wr, int wc, int lane, const f32x4 (&acc)[8][4], char* smem) {
  if (!GEGLU && p.rcs) {
    epi8p_rope(p, m0, n0, wr, wc, lane, acc, smem);
    return;
  }
  const int g4 = 4 * (lane >> 4), rl = lane & 15;
  if (GEGLU) {
    if (m0 + BT <= p.M && n0 + BT / 2 <= p.geglu_I && p.aux) {
      // h and g staged through the two 64 KiB LDS images (16-B row stores), u stored straight from the
      // accumulators (8 B per lane) in the same pass: one image round instead of two (u needs no LDS round
      // trip of its own; 4.03 vs 4.08-4.24 ms at 35328 x 32768 x 2048, bitwise equal,
      // profiles/r04/geglu_epi_ab.log; all three through direct 8-B stores measured 4.64 ms)
#pragma unroll
      for (int rb = 0; rb < 8; ++rb) {
        const int64_t m = m0 + wr * 128 + rb * 16 + rl;
        bf16_t* Ur = p.aux + m * p.ld_aux + p.geglu_I + n0 + wc * 32 + g4;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          float gg[4], hh[4], uu[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            gg[r] = acc[rb][j][r] * p.alpha;
            uu[r] = acc[rb][2 + j][r] * p.alpha;
            hh[r] = gelu_tanh(gg[r]) * uu[r];
          }
          const int row = wr * 128 + rb * 16 + rl, col = wc * 32 + j * 16 + g4;
          img_put(smem, row, col, u32x2{pack2bf(hh[0], hh[1]), pack2bf(hh[2], hh[3])});
          img_put(smem + 65536, row, col, u32x2{pack2bf(gg[0], gg[1]), pack2bf(gg[2], gg[3])});
          *reinterpret_cast<u32x2*>(Ur + j * 16) = pk4(uu);
        }
      }
      lds_sync();
      img_flush(smem, reinterpret_cast<bf16_t*>(p.C) + cofs + m0 * p.ldc + n0, p.ldc);
      img_flush(smem + 65536, p.aux + m0 * p.ld_aux + n0, p.ld_aux);
      return;
    }
#pragma unroll
    for (int rb = 0; rb < 8; ++rb) {
      const int64_t m = m0 + wr * 128 + rb * 16 + rl;
#pragma unroll
      for (int j = 0; j < 2; ++j) store_geglu4(p, cofs, m, n0 + wc * 32 + j * 16 + g4, acc[rb][j], acc[rb][2 + j]);
    }
    return;
  }
  const int64_t m = m0 + wr * 128 + (lane & 15), nb = n0 + wc * 64 + 4 * (lane >> 4);
  if (m0 + BT <= p.M && n0 + BT <= p.N) {
    switch (fast_mode(p)) {
      case FM_STORE: {  // two 256 x 128 images (columns 0..127 | 128..255), one pass
        float bias[4][4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
          if (p.bias) {
            unpack4(*reinterpret_cast<const u32x2*>(p.bias + nb + cb * 16), bias[cb]);
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) bias[cb][r] = 0.f;
          }
        }
        char* img = smem + (wc >> 1) * 65536;
#pragma unroll
        for (int rb = 0; rb < 8; ++rb)
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = acc[rb][cb][r] * p.alpha + bias[cb][r];
            img_put(img, wr * 128 + rb * 16 + rl, (wc & 1) * 64 + cb * 16 + g4, u32x2{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])});
          }
        lds_sync();
        bf16_t* C = reinterpret_cast<bf16_t*>(p.C) + cofs + m0 * p.ldc + n0;
        img_flush(smem, C, p.ldc);
        img_flush(smem + 65536, C + 128, p.ldc);
        break;
      }
      case FM_F32: epi8p_fast<FM_F32>(p, cofs, rofs, m, nb, acc); break;
      case FM_DACT: epi8p_staged<FM_DACT>(p, cofs, rofs, m0, n0, wr, wc, lane, acc, smem); break;
      case FM_DGEGLU: epi8p_staged<FM_DGEGLU>(p, cofs, rofs, m0, n0, wr, wc, lane, acc, smem); break;
      default: epi8p_staged<FM_BF16>(p, cofs, rofs, m0, n0, wr, wc, lane, acc, smem); break;
    }
    return;
  }
  // edge tile: park each half of the wave's accumulators in its own 16 KiB of the (now idle) LDS
  // and run ONE runtime-general group store in a rolled loop (lane-private slots: no barrier)
  f32x4* park = reinterpret_cast<f32x4*>(smem) + (wr * 4 + wc) * 1024 + lane;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int g = 0; g < 16; ++g) park[g * 64] = acc[half * 4 + (g >> 2)][g & 3];
#pragma unroll 1
    for (int g = 0; g < 16; ++g)
      store_out4_rt(p, cofs, rofs, m + (half * 4 + (g >> 2)) * 16, nb + (g & 3) * 16, park[g * 64]);
  }
}

// F8: fp8 (OCP e4m3) A and B, both k-contiguous, staged by the same byte-identical pipeline: the
// caller passes K, lda, ldb in units of 2 codes ("bf16-sized" elements), so a 64-unit K-tile is 128
// codes, and each (row block, column block) of a K-tile is ONE v_mfma_f32_16x16x128_f8f6f4 on the two
// bf16-shaped fragments of that tile concatenated (lane group g: codes 16g..16g+15 and 64+16g..
// 64+16g+15 of the tile on BOTH operands -- the same k set, so the sum is the plain dot product) at
// twice the bf16 MFMA rate.  The per-row activation scale (p.rs) multiplies the accumulators after
// the main loop (before the split-tail partials are written, so the tail sum stays linear); the
// weight scale is alpha.
// EXT (rank extension, KTAIL instantiation, whole tiles only): the ceil(K2 / 64) K-tiles of A2 / B2 follow the
// ceil(K / 64) main ones through the same pipeline -- only the DMA source of a tile changes -- and the K-tail
// clamping / masking applies to the last tile of EACH range (K % 8 == 0; K2 % 8 == 0, K2 >= 8).
template <bool AKC, bool BKC, bool GEGLU, bool KTAIL, bool F8, bool EXT = false>
__device__ __forceinline__ void gemm8p_body(const GemmP& p) {
  static_assert(!EXT || (KTAIL && !F8), "rank extension: bf16, tail-capable instantiation");
  static_assert(AKC, "a k-strided A takes gemm8k_kernel (use_khalf)");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nk1 = (int)((p.K + 63) / 64);  // main K-tiles
  const int nk_all = EXT ? nk1 + (int)((p.K2 + 63) / 64) : nk1;
  int lid = blockIdx.x, piece = -1, kt0 = 0, nk = nk_all;
  if (p.tail_s && lid >= p.dp_tiles) {  // split tail: one K-piece of a leftover tile
    const int u = lid - p.dp_tiles;
    piece = u;
    lid = p.dp_tiles + u / p.tail_s;
    kt0 = (u % p.tail_s) * p.tail_kt;
    nk = min(nk_all - kt0, p.tail_kt);
  }
  int tm, tn;
  tile_coords(lid, p.tiles_m * p.tiles_n, p.tiles_m, p.tiles_n, tm, tn, p.group);
  const int64_t m0 = (int64_t)tm * BT;
  const int64_t n0 = GEGLU ? (int64_t)tn * (BT / 2) : (int64_t)tn * BT;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int64_t z = blockIdx.y;
  const int64_t zo = z / p.batch_inner, zi = z % p.batch_inner;
  const bf16_t* Ab = p.A + zo * p.sAo + zi * p.sAi;
  const bf16_t* Bb = p.B + zo * p.sBo + zi * p.sBi;

  // pieces: 0 = A region 0, 1 = B region 0, 2 = B region 1, 3 = A region 1
  const bf16_t* src[4][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    src[0][i] = p8_src<AKC, true, false>(Ab, p.lda, 0, i, t, m0, p.M, 0);
    src[3][i] = p8_src<AKC, true, false>(Ab, p.lda, 1, i, t, m0, p.M, 0);
    src[1][i] = p8_src<BKC, false, GEGLU>(Bb, p.ldb, 0, i, t, n0, p.N, p.geglu_I);
    src[2][i] = p8_src<BKC, false, GEGLU>(Bb, p.ldb, 1, i, t, n0, p.N, p.geglu_I);
  }
  const int64_t stepA = AKC ? 64 : 64 * p.lda;
  const int64_t stepB = BKC ? 64 : 64 * p.ldb;
  // extension sources of the same lanes (K-tile kt >= nk1 reads tile kt - nk1 of A2 / B2)
  // (these 16 VGPRs push the EXT instantiations from 236 to 256 VGPRs with 11-25 spilled: profiles/lora/README.txt)
  const bf16_t* src2[4][2];
  const int64_t stepA2 = AKC ? 64 : 64 * p.lda2;
  const int64_t stepB2 = BKC ? 64 : 64 * p.ldb2;
  if (EXT) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      src2[0][i] = p8_src<AKC, true, false>(p.A2, p.lda2, 0, i, t, m0, p.M, 0);
      src2[3][i] = p8_src<AKC, true, false>(p.A2, p.lda2, 1, i, t, m0, p.M, 0);
      src2[1][i] = p8_src<BKC, false, GEGLU>(p.B2, p.ldb2, 0, i, t, n0, p.N, p.geglu_I);
      src2[2][i] = p8_src<BKC, false, GEGLU>(p.B2, p.ldb2, 1, i, t, n0, p.N, p.geglu_I);
    }
  }
  if (kt0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      src[0][i] += kt0 * stepA;
      src[3][i] += kt0 * stepA;
      src[1][i] += kt0 * stepB;
      src[2][i] += kt0 * stepB;
    }
  }
  constexpr int lds_off[4] = {0, 2 * P8_REG, 3 * P8_REG, P8_REG};
  // K % 64 != 0: the last K-tile has krem valid k; every lane's source is clamped into the
  // tensor (finite data) and the A fragments of k >= krem are zeroed before the MFMAs.
  // (KTAIL = false instantiations assume K % 64 == 0 and carry none of this code; a K-piece
  // that does not end the reduction has no tail)
  const int krem = EXT ? (int)(p.K2 - (int64_t)(nk_all - nk1 - 1) * 64)
                       : (KTAIL && kt0 + nk == nk_all) ? (int)(p.K - (int64_t)(nk_all - 1) * 64) : 64;  // 1..64
  const int krem1 = EXT ? (int)(p.K - (int64_t)(nk1 - 1) * 64) : 64;  // EXT: valid k of the last MAIN tile
  auto issue = [&](int piece, int kt) {
    char* dst = smem + (kt & 1) * P8_BUF + lds_off[piece] + wave * 1024;
    const bool isA = piece == 0 || piece == 3;
    const int64_t step = isA ? stepA : stepB;
    const bool kc = isA ? AKC : BKC;
    const int region = (piece == 3 || piece == 2) ? 1 : 0;
    const bool ext = EXT && kt >= nk1;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const bf16_t* g = ext ? src2[piece][i] + (kt - nk1) * (isA ? stepA2 : stepB2) : src[piece][i] + kt * step;
      if constexpr (EXT) {  // the last tile of the main range and of the extension range may both be partial
        const int kr = kt == nk1 - 1 ? krem1 : (kt == nk - 1 ? krem : 64);
        if (kr < 64) {
          if (kc) {
            const int r = i * 64 + (t >> 3);
            const int kl = 8 * ((t & 7) ^ ((r >> 1) & 7));
            if (kl >= kr) g -= kl - (kr - 8);
          } else {
            const int kl = region * 32 + i * 16 + (t >> 5);
            if (kl >= kr) g -= (int64_t)(kl - (kr - 1)) * (ext ? (isA ? p.lda2 : p.ldb2) : (isA ? p.lda : p.ldb));
          }
        }
      } else if (KTAIL && krem < 64 && kt == nk - 1) {
        if (kc) {  // this lane's 8 k: 8 * chunk within the tile
          const int r = i * 64 + (t >> 3);
          const int kl = 8 * ((t & 7) ^ ((r >> 1) & 7));
          if (kl >= krem) g -= kl - (krem - 8);
        } else {   // this lane's k-row within the tile
          const int kl = region * 32 + i * 16 + (t >> 5);
          if (kl >= krem) g -= (int64_t)(kl - (krem - 1)) * (isA ? p.lda : p.ldb);
        }
      }
      glds16(g, dst + i * 8192);
    }
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 af[4][2], bf[2][2][2];  // A quadrant rows (4 x 16) x kk;  B [bh][2 x 16 cols][kk]
  auto mask_tail_a = [&](int kt) {
    if constexpr (EXT) {
      const int kr = kt == nk1 - 1 ? krem1 : (kt == nk - 1 ? krem : 64);
      if (kr < 64) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk)
            if (kk * 32 + 8 * (lane >> 4) >= kr) af[i][kk] = bf16x8{};
      }
    } else if (KTAIL && krem < 64 && kt == nk - 1) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          if (kk * 32 + 8 * (lane >> 4) >= krem) af[i][kk] = bf16x8{};
    }
  };

  auto read_a = [&](const char* buf, int ah) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        af[i][kk] = AKC ? frag<true>(buf + ah * P8_REG, wr * 4 + i, kk, lane)
                        : frag_tr_asm<512>(buf, wr * 8 + ah * 4 + i, kk, lane);
  };
  auto read_b = [&](const char* buf, int bh) {
    const char* reg = buf + 2 * P8_REG + (wc >> 1) * P8_REG;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        bf[bh][j][kk] = BKC ? frag<true>(reg, (wc & 1) * 4 + bh * 2 + j, kk, lane)
                            : frag_tr_asm<512>(buf + 2 * P8_REG, wc * 4 + bh * 2 + j, kk, lane);
  };
  auto mfma_quad = [&](int ah, int bh) {
    __builtin_amdgcn_s_setprio(1);
    if (F8) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[ah * 4 + i][bh * 2 + j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              cat_f8(bf[bh][j][0], bf[bh][j][1]), cat_f8(af[i][0], af[i][1]), acc[ah * 4 + i][bh * 2 + j], 0, 0, 0, 0,
              0, 0);
    } else {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[ah * 4 + i][bh * 2 + j] =
                __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[bh][j][kk], af[i][kk], acc[ah * 4 + i][bh * 2 + j], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
  };

  // Two sections per K-tile (B either way -- a k-strided B is read whole in section 0 through transposed loads):
  // section 0 reads A region 0 and all of B (16 fragment loads) and runs quadrants (0,0), (0,1); section 1 reads
  // A region 1 (8) and runs (1,1), (1,0).  32 MFMAs per section against the other row group's reads; the older
  // four-phase schedule front-loaded 12 of its 24 loads into one 16-MFMA phase, and its loads, not its DMA, set
  // that phase's length (profiles/r05/feed_ab_*.log).  DMA: A1(kt+1) in section 0 (its region was last read
  // in section 1 of kt-1), A0 | B0 | B1 (kt+2) in section 1 (last read in section 0 of kt).  Waits (2 DMA
  // instructions per piece): section 0 retires A1(kt) (4 newer pieces), section 1 retires tile kt+1's
  // section-0 pieces (4 newer, or only A1(kt+1) on the next-to-last tile); each is followed by the
  // barrier the next reader of those regions passes.
  issue(0, 0);
  issue(1, 0);
  issue(2, 0);
  issue(3, 0);
  if (nk > 1) {
    issue(0, 1);
    issue(1, 1);
    issue(2, 1);
    PZ_WAIT_VM(8);
  } else {
    PZ_WAIT_VM(2);
  }
  PZ_RAW_BARRIER();
  if (wr == 1) PZ_RAW_BARRIER();  // stagger: row-1 waves run one barrier behind
  for (int kt = 0; kt < nk; ++kt) {
    const char* buf = smem + (kt & 1) * P8_BUF;
    const bool n1 = kt + 1 < nk, n2 = kt + 2 < nk;
    // section 0: quadrants (0,0), (0,1)
    if (n1) issue(3, kt + 1);
    read_a(buf, 0);
    read_b(buf, 0);
    read_b(buf, 1);
    if (n1) PZ_WAIT_VM(8);
    else PZ_WAIT_VM(0);
    PZ_WAIT_LGKM0();
    PZ_RAW_BARRIER();
    mask_tail_a(kt);
    mfma_quad(0, 0);
    mfma_quad(0, 1);
    PZ_RAW_BARRIER();
    // section 1: quadrants (1,1), (1,0)
    if (n2) {
      issue(0, kt + 2);
      issue(1, kt + 2);
      issue(2, kt + 2);
    }
    read_a(buf, 1);
    if (n2) PZ_WAIT_VM(8);
    else if (n1) PZ_WAIT_VM(2);
    PZ_WAIT_LGKM0();
    PZ_RAW_BARRIER();
    mask_tail_a(kt);
    mfma_quad(1, 1);
    mfma_quad(1, 0);
    PZ_RAW_BARRIER();
  }
  if (wr == 0) PZ_RAW_BARRIER();
  if (F8 && p.rs) {  // per-row activation scale: lane rows m0 + wr*128 + 16 rb + (lane & 15)
#pragma unroll
    for (int rb = 0; rb < 8; ++rb) {
      const int64_t row = min(m0 + wr * 128 + 16 * rb + (lane & 15), p.M - 1);
      const float sr = p.rs[row];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) acc[rb][cb] *= sr;
    }
  }

  if (piece >= 0) {  // split tail: raw partial sums, summed + epilogued by gemm8p_tail_epilogue
    f32x4* W = reinterpret_cast<f32x4*>(p.ws) + (int64_t)piece * (32 * NT2);
#pragma unroll
    for (int rb = 0; rb < 8; ++rb)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) W[(rb * 4 + cb) * NT2 + t] = acc[rb][cb];
    return;
  }
  epilogue8p<GEGLU>(p, zo * p.sCo + zi * p.sCi, zo * p.sRo + zi * p.sRi, m0, n0, wr, wc, lane, acc, smem);
}

template <bool AKC, bool BKC, bool GEGLU, bool KTAIL>
__global__ void __launch_bounds__(NT2, 1) gemm8p_kernel(GemmP p) {
  gemm8p_body<AKC, BKC, GEGLU, KTAIL, false>(p);
}

// ... with the rank extension (pz_gemm_args.K2 > 0, pz_qkv_rope_args.K2 > 0)
template <bool AKC, bool BKC, bool GEGLU>
__global__ void __launch_bounds__(NT2, 1) gemm8p_x_kernel(GemmP p) {
  gemm8p_body<AKC, BKC, GEGLU, true, false, true>(p);
}

// fp8 e4m3 x e4m3 (W8A8) instantiation of the 8-phase kernel (C5 prefill MLP GEMMs)
template <bool GEGLU, bool KTAIL>
__global__ void __launch_bounds__(NT2, 1) gemm8p_f8_kernel(GemmP p) {
  gemm8p_body<true, true, GEGLU, KTAIL, true>(p);
}

// ---- k-half variant of the ping-pong kernel -----------------------------------
// Same tile (256 x 256 x 64, 8 waves of 128 x 64), same accumulator layout, epilogue and split
// tail as gemm8p_kernel, but each K-tile is consumed in TWO segments per wave -- k 0..31 then
// k 32..63, each 32 MFMAs over the whole 128 x 64 wave tile -- instead of four 16-MFMA quadrant
// segments: half the barriers per K-tile and twice the matrix work beside each partner's
// LDS-read segment.  LDS regions are k-halves (per buffer: A h0 | A h1 | B h0 | B h1, 16 KiB
// each): k-contiguous images are [256 rows][32 k] (64-B rows, 16-B chunk c of row r at
// c ^ 3*((r >> 3) & 1): conflict-free ds_read_b128), k-strided ones the [32 k][256 rows] images of
// gemm8p_kernel.  Region (kt, h) is refilled with tile kt + 2 as soon as both wave groups have read
// it (h0 in segment 2 of kt, h1 in segment 0 of kt + 1): ~1.5 K-tiles of loads stay in flight.
constexpr int KH_REG = 16384;

template <bool GEGLU>
__device__ __forceinline__ int64_t kh_rowB(int v, int64_t row0, int64_t R, int64_t gI) {
  if (GEGLU) {  // virtual column v: wave (v >> 6), gate/up (v >> 5 & 1)
    int64_t g = row0 + (v >> 6) * 32 + (v & 31);
    g = g < gI ? g : gI - 1;
    return ((v >> 5) & 1) ? gI + g : g;
  }
  const int64_t g = row0 + v;
  return g < R ? g : R - 1;
}

// per-thread global source of DMA instruction i (0/1) of the k-half-0 region image of an operand
template <bool KC, bool GEGLU>
__device__ __forceinline__ const bf16_t* kh_src(const bf16_t* base, int64_t ld, int i, int t, int64_t row0,
                                                int64_t R, int64_t gI) {
  if (KC) {
    const int r = i * 128 + (t >> 2);
    const int ch = (t & 3) ^ (3 * ((r >> 3) & 1));
    return base + kh_rowB<GEGLU>(r, row0, R, gI) * ld + 8 * ch;
  } else {
    const int k = i * 16 + (t >> 5);
    const int c = (t & 31) ^ (sw_tr(k) >> 1);
    int64_t g = row0 + 8 * c;
    g = g <= R - 8 ? g : R - 8;
    return base + (int64_t)k * ld + g;
  }
}

template <bool KC>
__device__ __forceinline__ bf16x8 kh_frag(const char* opbase, int h, int rb, int lane) {
  if (KC) {
    const char* reg = opbase + h * KH_REG;
    const int r = rb * 16 + (lane & 15);
    const int ch = lane >> 4;
    return *reinterpret_cast<const bf16x8*>(reg + r * 64 + ((ch ^ (3 * ((r >> 3) & 1))) << 4));
  } else {
    return frag_tr_asm<512>(opbase, rb, h, lane);  // k-half h = k-rows 32h.. at 16 KiB * h
  }
}

template <bool AKC, bool BKC, bool GEGLU, bool KTAIL>
__global__ void __launch_bounds__(NT2, 1) gemm8k_kernel(GemmP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nk_all = (int)((p.K + 63) / 64);
  int lid = blockIdx.x, piece = -1, kt0 = 0, nk = nk_all;
  if (p.tail_s && lid >= p.dp_tiles) {
    const int u = lid - p.dp_tiles;
    piece = u;
    lid = p.dp_tiles + u / p.tail_s;
    kt0 = (u % p.tail_s) * p.tail_kt;
    nk = min(nk_all - kt0, p.tail_kt);
  }
  int tm, tn;
  tile_coords(lid, p.tiles_m * p.tiles_n, p.tiles_m, p.tiles_n, tm, tn, p.group);
  const int64_t m0 = (int64_t)tm * BT;
  const int64_t n0 = GEGLU ? (int64_t)tn * (BT / 2) : (int64_t)tn * BT;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int64_t z = blockIdx.y;
  const int64_t zo = z / p.batch_inner, zi = z % p.batch_inner;
  const bf16_t* Ab = p.A + zo * p.sAo + zi * p.sAi;
  const bf16_t* Bb = p.B + zo * p.sBo + zi * p.sBi;

  const int64_t stepA = AKC ? 64 : 64 * p.lda;
  const int64_t stepB = BKC ? 64 : 64 * p.ldb;
  const int64_t halfA = AKC ? 32 : 32 * p.lda;
  const int64_t halfB = BKC ? 32 : 32 * p.ldb;
  const bf16_t* srcA[2];
  const bf16_t* srcB[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    srcA[i] = kh_src<AKC, false>(Ab, p.lda, i, t, m0, p.M, 0) + kt0 * stepA;
    srcB[i] = kh_src<BKC, GEGLU>(Bb, p.ldb, i, t, n0, p.N, p.geglu_I) + kt0 * stepB;
  }
  const int krem = (KTAIL && kt0 + nk == nk_all) ? (int)(p.K - (int64_t)(nk_all - 1) * 64) : 64;
  // K % 64 != 0: every lane's source of the last K-tile is clamped into the tensor (finite data)
  // and the A fragments of k >= krem are zeroed before the MFMAs
  auto clamp_tail = [&](const bf16_t* g, bool kc, int h, int i, int64_t ld, int kt) {
    if (KTAIL && krem < 64 && kt == nk - 1) {
      if (kc) {
        const int r = i * 128 + (t >> 2);
        const int kl = 32 * h + 8 * ((t & 3) ^ (3 * ((r >> 3) & 1)));
        if (kl >= krem) g -= kl - (krem - 8);
      } else {
        const int kl = 32 * h + i * 16 + (t >> 5);
        if (kl >= krem) g -= (int64_t)(kl - (krem - 1)) * ld;
      }
    }
    return g;
  };
  // k-half h of K-tile kt (both operands): 2 + 2 DMA instructions per wave
  auto issue = [&](int kt, int h) {
    char* dst = smem + (kt & 1) * P8_BUF + h * KH_REG + wave * 1024;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      glds16(clamp_tail(srcA[i] + kt * stepA + h * halfA, AKC, h, i, p.lda, kt), dst + i * 8192);
      glds16(clamp_tail(srcB[i] + kt * stepB + h * halfB, BKC, h, i, p.ldb, kt), dst + 2 * KH_REG + i * 8192);
    }
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 af[8], bfr[4];
  auto read_frags = [&](const char* buf, int h) {
#pragma unroll
    for (int i = 0; i < 8; ++i) af[i] = kh_frag<AKC>(buf, h, wr * 8 + i, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) bfr[j] = kh_frag<BKC>(buf + 2 * KH_REG, h, wc * 4 + j, lane);
  };
  auto mask_tail_a = [&](int kt, int h) {
    if (KTAIL && krem < 64 && kt == nk - 1) {
      if (32 * h + 8 * (lane >> 4) >= krem) {
#pragma unroll
        for (int i = 0; i < 8; ++i) af[i] = bf16x8{};
      }
    }
  };
  auto mfma_half = [&]() {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };

  // issue order: (0,0) (0,1) (1,0) | per tile kt: (kt+1,1) in segment 0, (kt+2,0) in segment 2.
  // Waits (4 DMA instructions per wave per k-half): segment 0 retires (kt,1), segment 2 retires
  // (kt+1,0); each is followed by the barrier the next reader of that region passes.
  issue(0, 0);
  issue(0, 1);
  if (nk > 1) {
    issue(1, 0);
    PZ_WAIT_VM(8);
  } else {
    PZ_WAIT_VM(4);
  }
  PZ_RAW_BARRIER();
  if (wr == 1) PZ_RAW_BARRIER();  // stagger: waves 4..7 run one barrier behind

  for (int kt = 0; kt < nk; ++kt) {
    const char* buf = smem + (kt & 1) * P8_BUF;
    const bool n1 = kt + 1 < nk, n2 = kt + 2 < nk;
    // segment 0: read k-half 0
    if (n1) issue(kt + 1, 1);
    read_frags(buf, 0);
    if (n1) PZ_WAIT_VM(8);
    else PZ_WAIT_VM(0);
    PZ_WAIT_LGKM0();
    PZ_RAW_BARRIER();
    // segment 1: MFMAs of k-half 0
    mask_tail_a(kt, 0);
    mfma_half();
    PZ_RAW_BARRIER();
    // segment 2: read k-half 1
    if (n2) issue(kt + 2, 0);
    read_frags(buf, 1);
    if (n2) PZ_WAIT_VM(8);
    else if (n1) PZ_WAIT_VM(4);
    PZ_WAIT_LGKM0();
    PZ_RAW_BARRIER();
    // segment 3: MFMAs of k-half 1
    mask_tail_a(kt, 1);
    mfma_half();
    PZ_RAW_BARRIER();
  }
  if (wr == 0) PZ_RAW_BARRIER();

  if (piece >= 0) {
    f32x4* W = reinterpret_cast<f32x4*>(p.ws) + (int64_t)piece * (32 * NT2);
#pragma unroll
    for (int rb = 0; rb < 8; ++rb)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) W[(rb * 4 + cb) * NT2 + t] = acc[rb][cb];
    return;
  }
  epilogue8p<GEGLU>(p, zo * p.sCo + zi * p.sCi, zo * p.sRo + zi * p.sRi, m0, n0, wr, wc, lane, acc, smem);
}

// Split tail, second pass: 16 blocks of 512 threads per leftover tile (one accumulator row-block rb and
// one column half each, so the partial sums stream through many CUs); thread t sums the tail_s
// partial accumulators it owned in gemm8p_kernel (fixed order) and applies the same epilogue.
template <bool GEGLU>
__global__ void __launch_bounds__(NT2) gemm8p_tail_epilogue(GemmP p) {
  const int tile = blockIdx.x >> 4, rb = (blockIdx.x >> 1) & 7, h = blockIdx.x & 1;
  int tm, tn;
  tile_coords(p.dp_tiles + tile, p.tiles_m * p.tiles_n, p.tiles_m, p.tiles_n, tm, tn, p.group);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wr = wave >> 2, wc = wave & 3;
  const f32x4* W = reinterpret_cast<const f32x4*>(p.ws) + (int64_t)tile * p.tail_s * (32 * NT2);
  // GeGLU pairs gate cb = h with up cb = h + 2; plain outputs take cb = 2h, 2h + 1
  const int c0 = GEGLU ? h : 2 * h, c1 = GEGLU ? h + 2 : 2 * h + 1;
  // pieces loaded PB at a time (2 PB loads in flight per thread), summed in piece order (deterministic)
  constexpr int PB = 8;
  const f32x4* W0 = W + (rb * 4 + c0) * NT2 + t;
  const f32x4* W1 = W + (rb * 4 + c1) * NT2 + t;
  auto sum_pieces = [&](f32x4& a0, f32x4& a1) {
    a0 = a1 = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int z = 0; z < p.tail_s; z += PB) {
      f32x4 v0[PB], v1[PB];
#pragma unroll
      for (int u = 0; u < PB; ++u) {
        const bool ok = z + u < p.tail_s;
        v0[u] = ok ? W0[(int64_t)(z + u) * (32 * NT2)] : f32x4{0.f, 0.f, 0.f, 0.f};
        v1[u] = ok ? W1[(int64_t)(z + u) * (32 * NT2)] : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < PB; ++u) {
        a0 += v0[u];
        a1 += v1[u];
      }
    }
  };
  const int64_t m = (int64_t)tm * BT + wr * 128 + rb * 16 + (lane & 15);
  f32x4 a0, a1;
  if (GEGLU) {
    sum_pieces(a0, a1);
    store_geglu4(p, 0, m, (int64_t)tn * (BT / 2) + wc * 32 + h * 16 + 4 * (lane >> 4), a0, a1);
  } else {
    const int64_t n = (int64_t)tn * BT + wc * 64 + 4 * (lane >> 4);
    // the epilogue's side inputs (residual, saved activation, bias) issued with the first pieces, not after the sum
    epi_dispatch(p, [&](auto em) {
      constexpr int EM = decltype(em)::value;
      Side s0, s1;
      epi_load4<EM>(p, 0, 0, m, n + c0 * 16, s0);
      epi_load4<EM>(p, 0, 0, m, n + c1 * 16, s1);
      const u32x2 b0 = epi_load_bias(p, n + c0 * 16), b1 = epi_load_bias(p, n + c1 * 16);
      sum_pieces(a0, a1);
      epi_store4<EM>(p, 0, 0, m, n + c0 * 16, a0, s0, b0);
      epi_store4<EM>(p, 0, 0, m, n + c1 * 16, a1, s1, b1);
    });
  }
}

// -------------------------------------------------------------------------
// Skinny GEMM for M <= 16 (inference denoise steps, B = 1..4): weights are
// streamed once straight into VGPRs (no LDS), a block of W waves per 16 output
// columns, K split into W contiguous ranges (one per wave, loads issued 8 / 4
// chunks ahead of their MFMAs so each lane keeps up to 8 x 16 B of weights in
// flight) and reduced through LDS.  W = 4/8/16 by K so every wave has >= 4
// chunks of 32.  Operands k-contiguous (nn.Linear weight layout).
// -------------------------------------------------------------------------
template <int W, int NC>
__global__ void __launch_bounds__(W * 64) gemm_skinny_kernel(GemmP p) {
  constexpr int SK_WAVES = W;
  __shared__ f32x4 red[SK_WAVES][64];
  __shared__ float redn[SK_WAVES][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool geglu = p.epi == PZ_EPI_GEGLU;
  const bool nrm = p.nw != nullptr;
  const int64_t ncols = geglu ? p.geglu_I : p.N;
  // NC < 16 output columns per block (more blocks for narrow outputs): the 16 MFMA columns repeat
  // the NC real ones (same addresses, no extra traffic) and only the first NC are stored
  const int64_t n0 = (int64_t)blockIdx.x * NC;
  const int64_t z = blockIdx.y;
  const int64_t zo = z / p.batch_inner, zi = z % p.batch_inner;
  const bf16_t* A = p.A + zo * p.sAo + zi * p.sAi;
  const bf16_t* B = p.B + zo * p.sBo + zi * p.sBi;
  const int64_t m = lane & 15;
  const int64_t nr = n0 + (lane & 15) % NC;
  const bool mok = m < p.M, nok = nr < ncols;
  const int64_t kchunks = p.K / 32;  // K % 32 == 0 required (host checked)
  f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};
  float ss = 0.f;
  const bf16_t* Arow = A + m * p.lda + 8 * (lane >> 4);
  const bf16_t* Brow = B + nr * p.ldb + 8 * (lane >> 4);
  const bf16_t* Brow2 = B + (p.geglu_I + nr) * p.ldb + 8 * (lane >> 4);
  const bf16_t* Wn = p.nw + 8 * (lane >> 4);
  const int64_t per = (kchunks + SK_WAVES - 1) / SK_WAVES;
  const int64_t kb = wave * per, ke = min(kchunks, kb + per);
  int64_t kc = kb;
  auto run = [&](auto U_) {
    constexpr int U = decltype(U_)::value;
    for (; kc + U <= ke; kc += U) {
      bf16x8 a[U], b[U], b2[U], wv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        a[u] = mok ? *reinterpret_cast<const bf16x8*>(Arow + (kc + u) * 32) : bf16x8{};
        b[u] = nok ? *reinterpret_cast<const bf16x8*>(Brow + (kc + u) * 32) : bf16x8{};
        if (geglu) b2[u] = nok ? *reinterpret_cast<const bf16x8*>(Brow2 + (kc + u) * 32) : bf16x8{};
        if (nrm) wv[u] = *reinterpret_cast<const bf16x8*>(Wn + (kc + u) * 32);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (nrm) {  // sum of squares of the raw row; the product takes x * (1 + w), rsqrt applied after
          const u32x4 xa = __builtin_bit_cast(u32x4, a[u]), xw = __builtin_bit_cast(u32x4, wv[u]);
          u32x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float x0 = __uint_as_float(xa[e] << 16), x1 = __uint_as_float(xa[e] & 0xffff0000u);
            const float w0 = __uint_as_float(xw[e] << 16), w1 = __uint_as_float(xw[e] & 0xffff0000u);
            ss += x0 * x0 + x1 * x1;
            o[e] = pack2bf(x0 * (1.f + w0), x1 * (1.f + w1));
          }
          a[u] = __builtin_bit_cast(bf16x8, o);
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[u], a[u], acc, 0, 0, 0);
        if (geglu) acc2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b2[u], a[u], acc2, 0, 0, 0);
      }
    }
  };
  run(std::integral_constant<int, 8>{});
  run(std::integral_constant<int, 4>{});
  run(std::integral_constant<int, 1>{});
  // D[n_local = 4*(lane>>4)+r][m = lane&15]
  red[wave][lane] = acc;
  if (nrm) {
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    if (lane < 16) redn[wave][lane] = ss;
  }
  __syncthreads();
  if (wave == 0) {
    for (int w = 1; w < SK_WAVES; ++w) acc += red[w][lane];
  }
  if (geglu) {
    __syncthreads();
    red[wave][lane] = acc2;
    __syncthreads();
    if (wave == 0)
      for (int w = 1; w < SK_WAVES; ++w) acc2 += red[w][lane];
  }
  if (wave != 0) return;
  const int64_t mm = lane & 15;
  if (mm >= p.M) return;
  float scale = p.alpha;
  if (nrm) {
    float t = 0.f;
    for (int w = 0; w < SK_WAVES; ++w) t += redn[w][mm];
    scale *= rsqrtf(t / (float)p.K + p.neps);
  }
  const int64_t n = n0 + 4 * (lane >> 4);
  const int64_t cofs = zo * p.sCo + zi * p.sCi;
  const int64_t rofs = zo * p.sRo + zi * p.sRi;
  for (int r = 0; r < 4; ++r) {
    const int64_t nn = n + r;
    if (4 * (lane >> 4) + r >= NC || nn >= ncols) continue;
    float x = acc[r] * scale;
    if (geglu) {
      const float g = x, u = acc2[r] * scale;
      if (p.aux) {
        p.aux[mm * p.ld_aux + nn] = f2bf(g);
        p.aux[mm * p.ld_aux + p.geglu_I + nn] = f2bf(u);
      }
      x = gelu_tanh(g) * u;
    } else {
      if (p.bias) x += bf2f(p.bias[nn]);
      if (p.epi == PZ_EPI_GELU || p.epi == PZ_EPI_SILU) {
        if (p.aux) p.aux[mm * p.ld_aux + nn] = f2bf(x);
        x = p.epi == PZ_EPI_GELU ? gelu_tanh(x) : silu(x);
      }
      if (p.resid) x += bf2f(p.resid[rofs + mm * p.ld_resid + nn]);
    }
    if (p.c_fp32) {
      float* Cp = reinterpret_cast<float*>(p.C) + cofs + mm * p.ldc + nn;
      *Cp = p.beta ? *Cp + x : x;
    } else {
      bf16_t* Cp = reinterpret_cast<bf16_t*>(p.C) + cofs + mm * p.ldc + nn;
      *Cp = f2bf(p.beta ? bf2f(*Cp) + x : x);
    }
  }
}

// -------------------------------------------------------------------------
// Small strided fp32-accumulate GEMM for the K=7 / N=7 action/proprio linears
// (SURVEY 2.2 "proprio enc / action dec": 0.03 GF).  One thread per output.
// -------------------------------------------------------------------------
__global__ void gemm_small_kernel(pz_small_gemm_args a) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.M * a.N) return;
  const int64_t m = idx / a.N, n = idx % a.N;
  const bf16_t* A = (const bf16_t*)a.A;
  const bf16_t* B = (const bf16_t*)a.B;
  float s = 0.f;
  for (int64_t k = 0; k < a.K; ++k)
    s += bf2f(A[m * a.sAm + k * a.sAk]) * bf2f(B[k * a.sBk + n * a.sBn]);
  s *= a.alpha;
  if (a.bias) s += bf2f(((const bf16_t*)a.bias)[n]);
  bf16_t* C = (bf16_t*)a.C + m * a.ldc + n;
  if (a.beta) s += bf2f(*C);
  *C = f2bf(s);
}

// Long-K / tiny-N case (action decoder, pizero.py:100-103: [rows, 1024] x [7, 1024]^T): one wave
// per output row, lanes split K in 16-B chunks (k-contiguous A and B), butterfly reduction.
constexpr int SMALL_NMAX = 8;
__global__ void __launch_bounds__(256) gemm_small_rowwave_kernel(pz_small_gemm_args a) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= a.M) return;
  const bf16_t* A = (const bf16_t*)a.A + m * a.sAm;
  const bf16_t* B = (const bf16_t*)a.B;
  float s[SMALL_NMAX];
#pragma unroll
  for (int n = 0; n < SMALL_NMAX; ++n) s[n] = 0.f;
  for (int64_t k = 8 * lane; k < a.K; k += 512) {
    const u32x4 xa = *reinterpret_cast<const u32x4*>(A + k);
    float x[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x[2 * e] = bf2f(xa[e] & 0xffff);
      x[2 * e + 1] = bf2f(xa[e] >> 16);
    }
#pragma unroll
    for (int n = 0; n < SMALL_NMAX; ++n) {
      if (n >= a.N) break;
      const u32x4 wb = *reinterpret_cast<const u32x4*>(B + n * a.sBn + k);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[n] += x[2 * e] * bf2f(wb[e] & 0xffff) + x[2 * e + 1] * bf2f(wb[e] >> 16);
    }
  }
#pragma unroll
  for (int n = 0; n < SMALL_NMAX; ++n) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[n] += __shfl_xor(s[n], off);
  }
  if (lane < a.N) {
    float v = 0.f;
#pragma unroll
    for (int n = 0; n < SMALL_NMAX; ++n)
      if (n == lane) v = s[n];
    v *= a.alpha;
    if (a.bias) v += bf2f(((const bf16_t*)a.bias)[lane]);
    bf16_t* C = (bf16_t*)a.C + m * a.ldc + lane;
    if (a.beta) v += bf2f(*C);
    *C = f2bf(v);
  }
}

}  // namespace

// ------------------------------------------------------------ launchers ----
// (the planner, pz_gemm and pz_gemm_kernel_name: pz_gemm_host.hip)

// split-K second pass over ncols output columns (GeGLU: the I gate / up pairs)
static int launch_splitk_epi(const GemmP& p, int64_t ncols, int S, hipStream_t st) {
  const int64_t work = p.M * ((ncols + 3) / 4);
  hipLaunchKernelGGL(splitk_epilogue_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, p, S);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}

int pz_splitk_epi_launch(const GemmP& p, int S, hipStream_t st) { return launch_splitk_epi(p, p.N, S, st); }

// 128-tile kernels: batch entries (or split-K slices) over blockIdx.y, or the XCD-grouped 1-D grid
template <auto KERN>
static int launch_tile(const GemmP& p, const Plan& pl, hipStream_t st) {
  const int smem = 4 * TILE_BYTES;
  pz_dyn_smem<KERN>(smem);
  const int64_t tiles = pl.tiles_m * pl.tiles_n, nz = pl.kind == PATH_SPLIT ? pl.splits : pl.batch;
  const dim3 grid = pl.batch_xcd ? dim3((unsigned)(tiles * nz)) : dim3((unsigned)tiles, (unsigned)nz);
  hipLaunchKernelGGL(KERN, grid, dim3(NT), smem, st, p);
  PZ_CHECK_LAUNCH();
  if (pl.kind == PATH_SPLIT) return launch_splitk_epi(p, pl.geglu ? p.geglu_I : p.N, pl.splits, st);
  return PZ_OK;
}

int pz_tile_launch(const GemmP& p, const Plan& pl, hipStream_t st) {
  if (pl.tag) return launch_tile<gemm_kernel<true, true, 4, 1>>(p, pl, st);
  return with_bool(pl.geglu, [&](auto geglu) {
    constexpr bool G = decltype(geglu)::value;
    constexpr int WM = G ? 4 : 2;
    return with_layout<G>(pl.akc, pl.bkc, [&](auto akc, auto bkc) {
      constexpr bool AKC = decltype(akc)::value, BKC = decltype(bkc)::value;
      // rank-extended form: whole K, batch 1
      if (pl.x) return launch_tile<gemm_x_kernel<AKC, BKC, WM>>(p, pl, st);
      return launch_tile<gemm_kernel<AKC, BKC, WM, 0>>(p, pl, st);
    });
  });
}

// 8-phase kernels: pl.units work units (whole tiles, then the K-pieces of the split tail and their merge)
template <auto KERN, bool GEGLU>
static int launch8p(const GemmP& p, const Plan& pl, hipStream_t st) {
  const int smem = 2 * P8_BUF;  // 128 KiB
  pz_dyn_smem<KERN>(smem);
  hipLaunchKernelGGL(KERN, dim3(pl.units, (unsigned)pl.batch), dim3(NT2), smem, st, p);
  PZ_CHECK_LAUNCH();
  if (pl.tail_s) {
    const int T = p.tiles_m * p.tiles_n;
    hipLaunchKernelGGL(gemm8p_tail_epilogue<GEGLU>, dim3((T - p.dp_tiles) * 16), dim3(NT2), 0, st, p);
    PZ_CHECK_LAUNCH();
  }
  return PZ_OK;
}

int pz_8p_launch(const GemmP& p, const Plan& pl, hipStream_t st) {
  return with_bool(pl.geglu, [&](auto geglu) {
    constexpr bool G = decltype(geglu)::value;
    if (pl.x)  // rank-extended form: whole tiles, batch 1, A k-contiguous
      return with_bkc<G>(pl.bkc, [&](auto bkc) {
        return launch8p<gemm8p_x_kernel<true, decltype(bkc)::value, G>, G>(p, pl, st);
      });
    return with_bool(pl.ktail, [&](auto ktail) {
      constexpr bool KT = decltype(ktail)::value;
      if (pl.fp8 == 1) return launch8p<gemm8p_f8_kernel<G, KT>, G>(p, pl, st);
      return with_layout<G>(pl.akc, pl.bkc, [&](auto akc, auto bkc) {
        constexpr bool AKC = decltype(akc)::value, BKC = decltype(bkc)::value;
        if constexpr (AKC)  // (gemm8p_kernel reads a k-contiguous A only; the planner never sends a k-strided A there)
          if (!pl.khalf) return launch8p<gemm8p_kernel<AKC, BKC, G, KT>, G>(p, pl, st);
        return launch8p<gemm8k_kernel<AKC, BKC, G, KT>, G>(p, pl, st);
      });
    });
  });
}

template <int W, int NC>
static int launch_skinny(const GemmP& p, const Plan& pl, hipStream_t st) {
  hipLaunchKernelGGL((gemm_skinny_kernel<W, NC>), dim3((unsigned)pl.tiles_n, (unsigned)pl.batch), dim3(W * 64), 0, st,
                     p);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}

int pz_skinny_launch(const GemmP& p, const Plan& pl, hipStream_t st) {
  return with_int<16, 8, 4>(pl.skinny_w, [&](auto w) {
    return with_int<4, 8, 16>(pl.skinny_nc, [&](auto nc) {
      return launch_skinny<decltype(w)::value, decltype(nc)::value>(p, pl, st);
    });
  });
}

extern "C" int pz_gemm_small(const pz_small_gemm_args* a, void* stream) {
  PZ_CHECK_ARG(a && a->A && a->B && a->C && a->M > 0 && a->N > 0 && a->K > 0, "pz_gemm_small: bad args");
  if (a->N <= SMALL_NMAX && a->K >= 256 && a->K % 8 == 0 && a->sAk == 1 && a->sBk == 1 && a->sAm % 8 == 0 &&
      a->sBn % 8 == 0 && PZ_ALIGNED(a->A, 16) && PZ_ALIGNED(a->B, 16)) {
    hipLaunchKernelGGL(gemm_small_rowwave_kernel, dim3((unsigned)((a->M + 3) / 4)), dim3(256), 0,
                       (hipStream_t)stream, *a);
    PZ_CHECK_LAUNCH();
    return PZ_OK;
  }
  const int64_t total = a->M * a->N;
  hipLaunchKernelGGL(gemm_small_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, *a);
  PZ_CHECK_LAUNCH();
  return PZ_OK;
}
