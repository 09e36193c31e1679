// The GEMM plan: which kernel, with which template arguments, on which grid.  make_plan (pz_gemm_host.hip) fills a
// Plan from a validated pz_gemm_args and the PZ_* switches; pz_gemm_kernel_name prints it and the launchers of the
// kernel files (pz_gemm.hip, pz_gemm_rows.hip, pz_gemm_tall.hip) launch it.  Nothing but make_plan decides.
#pragma once

#include <type_traits>

#include "pz_gemm_epi.h"

// tile sizes the planner counts in: the 128-tile kernel's BM x BN x BK, the 8-phase kernels' BT x BT tile and NT2
// threads (pz_gemm.hip)
constexpr int BM = 128, BN = 128, BK = 64;
constexpr int BT = 256, NT2 = 512;

// PATH_NONE: no kernel takes the arguments (W8A16 above 64 rows outside the row-slab shapes); pz_gemm rejects them
enum PathKind {
  PATH_SKINNY, PATH_256, PATH_TILE, PATH_SPLIT, PATH_GEMV, PATH_SKINNY64, PATH_ROWS, PATH_TALL, PATH_NONE
};
struct Plan {
  PathKind kind;
  bool akc, bkc, geglu;
  bool x;    // rank-extended (_x) kernel forms: K2 > 0
  int fp8;   // 1 = W8A8 (both operands e4m3 codes), 2 = W8A16 (e4m3 weight codes), 0 = bf16
  int wm, tag, skinny_w, skinny_nc, skinny_mb;
  int splits;  // split-K slices of the 128-tile, tall-tile and skinny-64 kernels (0: whole K)
  int64_t ksplit, ldw, tiles_m, tiles_n;
  int64_t batch;   // grid rows of the batched kernels (pz_gemm_args.batch)
  bool batch_xcd;  // 128-tile kernel: XCD-grouped 1-D grid (GemmP::batch_xcd; PZ_GEMM_BATCH_XCD)
  bool sk_fused;   // skinny-64 split-K: partials summed in the launch (else by splitk_epilogue_kernel)
  // 8-phase kernels: k-half main loop (gemm8k_kernel), K % 64 != 0, tile-order super-row height, work units
  bool khalf, ktail;
  int group, units;
  int dp_tiles, tail_s, tail_kt;  // 8-phase split tail (tail_s == 0: none)
  int rows_w, rows_tnb, rows_tmb;  // row-slab kernel: waves, 16-column / 16-row blocks per tile
  int rows_f8;                     // ... with e4m3 weight codes: 1 = W8A16, 2 = W8A8 (both operands codes)
  int tall_mi;                     // tall-tile kernel: 64 * tall_mi rows per tile (4 | 5)
  int gemv_mr;                     // GEMV kernel: rows per workgroup (4 | 8)
};

// ---- launchers: each launches what the plan states and decides nothing itself ----
// skinny kernel (pz_gemm.hip): M <= 16 rows, skinny_w waves, skinny_nc columns per block
int pz_skinny_launch(const GemmP& p, const Plan& pl, hipStream_t st);
// 128-tile kernel (pz_gemm.hip), its rank-extended form and its split-K pair
int pz_tile_launch(const GemmP& p, const Plan& pl, hipStream_t st);
// 8-phase 256-tile kernels (pz_gemm.hip): bf16 (region or k-half main loop), rank-extended and fp8 W8A8 forms,
// each followed by the tail merge when the plan splits the leftover tiles
int pz_8p_launch(const GemmP& p, const Plan& pl, hipStream_t st);
// row-slab kernels (pz_gemm_rows.hip): rows_w waves, rows_tnb 16-column blocks per 64-row tile
int pz_rows_launch(const GemmP& p, const Plan& pl, hipStream_t st);
// skinny-64 kernel (pz_gemm_rows.hip): M <= 64 rows (16 < M bf16, any with fp8 weights: W8A16), skinny_w waves,
// 16 columns per block, skinny_mb 16-row blocks
int pz_sk64_launch(const GemmP& p, const Plan& pl, hipStream_t st);
// tall-tile kernel (pz_gemm_tall.hip): 64 * tall_mi rows per tile, k-contiguous A and B, plain epilogues,
// split-K over blockIdx.y when splits > 1
int pz_tall_launch(const GemmP& p, const Plan& pl, hipStream_t st);
// split-K second pass (pz_gemm.hip): C = epilogue(sum of the S fp32 partial slabs in p.ws)
int pz_splitk_epi_launch(const GemmP& p, int S, hipStream_t st);

// ---- run-time selectors -> template arguments ----
template <bool V>
using pz_bool = std::integral_constant<bool, V>;
template <int V>
using pz_int = std::integral_constant<int, V>;

template <class F>
int with_bool(bool b, F&& f) {
  return b ? f(pz_bool<true>{}) : f(pz_bool<false>{});
}
// f(pz_int<V>) for the first listed V that equals v, the last one when none does
template <int V0, int... Vs, class F>
int with_int(int v, F&& f) {
  if constexpr (sizeof...(Vs) > 0)
    if (v != V0) return with_int<Vs...>(v, f);
  return f(pz_int<V0>{});
}
// f(bkc) / f(akc, bkc) with the operand layouts as constants.  The GeGLU kernels read B = [gate; up] k-contiguous
// only: with GEGLU no k-strided-B form is instantiated.
template <bool GEGLU, class F>
int with_bkc(bool bkc, F&& f) {
  if constexpr (GEGLU) return f(pz_bool<true>{});
  else return with_bool(bkc, f);
}
template <bool GEGLU, class F>
int with_layout(bool akc, bool bkc, F&& f) {
  return with_bool(akc, [&](auto a) { return with_bkc<GEGLU>(bkc, [&](auto b) { return f(a, b); }); });
}

// raise KERN's dynamic LDS limit, once per kernel instantiation per process
template <auto KERN>
void pz_dyn_smem(int bytes) {
  static const hipError_t once =
      hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  (void)once;
}
