// Host side of pz_gemm (no kernel here): argument validation, the planner (make_plan: which kernel, with which
// template arguments, on which grid), pz_gemm_kernel_name, which prints a plan, and pz_gemm / pz_gemm_qkv_rope, which
// fill the kernels' argument block and hand plan and block to the launcher of the planned kernel (pz_gemm_plan.h).
// Every PZ_* switch of the GEMM path is read while the plan is made.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pz_gemm_plan.h"

static thread_local char g_err[512];
void pz_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* pz_last_error(void) { return g_err; }

extern "C" int pz_abi_version(void) { return PZ_ABI_VERSION; }

// main loop of the 256-tile kernels: k-half segments (gemm8k_kernel) when an operand is k-strided,
// region sections (gemm8p_kernel) when both are k-contiguous -- there the k-half images' 64-B row
// pieces cost more than the halved barrier count saves (measured on every Pi0 NT shape) -- and, since the
// two-section loop (round 5), for the micro-batch's NN dgrads (A k-contiguous, B k-strided; >= 16384 rows) with
// >= 4096 output columns or a reduction >= 4096: 2-4 % faster there, 2.5 % slower at 2048 x 2048
// (profiles/r05/nn_main_ab.log; smaller row counts not measured, left on the k-half kernel).  Micro-batch census:
// gate|up dgrad 128.5 vs 136.2 ms, down-proj DGEGLU dgrad 90.5 vs 94.1 ms, all GEMMs 854.6 vs 865.5 ms
// (profiles/r05/census_nn_routing_ab.log).
static bool use_khalf(bool akc, bool bkc, int64_t m, int64_t n, int64_t k) {
  if (akc && !bkc && m >= 16384 && (n >= 4096 || k >= 4096)) return false;
  return !(akc && bkc);
}

namespace {
// skinny-64 split-K: partials summed in the launch (default) or by splitk_epilogue_kernel (PZ_SK64_FUSED=0)
static bool sk64_two_launch() {
  const char* e = getenv("PZ_SK64_FUSED");
  return e && e[0] == '0';
}

// Wave quantisation of the 8-phase kernel (one 256x256 tile per CU at a time): T = q*G + r tiles
// leave the last round r/G full.  Split each of the r leftover tiles into s K-pieces (s*r <= G)
// so the last round takes ~1/s of a tile time; partial sums go through the fp32 workspace.
// q == 0 (fewer tiles than CUs, e.g. weight gradients of small layers) is the same split.
void plan_tail(Plan& pl, const pz_gemm_args* a) {
  if (a->batch != 1 || !a->workspace || !PZ_ALIGNED(a->workspace, 16)) return;
  const char* e = getenv("PZ_GEMM_TAIL");  // "0": whole tiles only (A/B runs; read per call)
  if (e && e[0] == '0') return;
  const int64_t G = pz_device_cus();
  const int64_t T = pl.tiles_m * pl.tiles_n;
  const int64_t q = T / G, r = T % G;
  const int64_t nk = (a->K + 63) / 64;
  // a leftover round at least half full runs about as fast as its K-pieces would (less contention);
  // after many rounds the workgroups no longer run in lockstep and the leftover tiles fill the gaps
  // (measured: split worse at q = 17, better at q <= 4)
  // (splitting a leftover round exactly half full -- micro-batch 128's SigLIP 1152-wide GEMMs, 640 tiles = 2 rounds +
  // 128 -- measured within noise: profiles/r04/siglip_1152_ab.txt)
  if (r == 0 || (q > 0 && 2 * r >= G) || q > 8) return;
  int64_t s = G / r;
  s = s < 16 ? s : 16;
  if (q == 0) {
    // the whole GEMM is the tail (weight gradients of the 1152-wide SigLIP layers: 70 / 85 / 25 tiles): the pieces
    // may take several rounds when that fills the CUs better.  Cost (us) = rounds(s) / s x nk x 1.8 (a 256 x 256 x 64
    // step at ~4.6 TF/s per CU) + r s x 0.1 (each piece's 256 KiB fp32 partial written and re-read, chip-wide):
    // 70 tiles x 1024 K-tiles -> 3 pieces in one 82 %-full round 635 us, 7 pieces in two 96 %-full rounds 576 us
    const int64_t smax = (int64_t)(a->ws_bytes / (32 * NT2 * 16)) / r;
    auto cost = [&](int64_t s2) { return (double)((r * s2 + G - 1) / G) / (double)s2 * (double)nk * 1.8 + r * s2 * 0.1; };
    double best = cost(s);
    for (int64_t s2 = s + 1; s2 <= 16 && s2 <= nk / 2 && s2 <= smax; ++s2) {
      const double c = cost(s2);
      if (c < best * 0.97) {
        best = c;
        s = s2;
      }
    }
  }
  // no split below 8 K-tiles: a piece writes (and the merge re-reads) a 256 KiB fp32 partial, which a short
  // reduction cannot amortise -- the K = 320 action-expert wgrad (8192 x 1024, 5 K-tiles) took 42.0 us with
  // 2 pieces per leftover tile vs 20.0 us whole (profiles/r03/shape_ab.log)
  s = s < nk / 2 ? s : nk / 2;
  if (s < 2 || nk < 8) return;
  const int64_t kt = (nk + s - 1) / s;
  s = (nk + kt - 1) / kt;
  if (s < 2 || r * s * (int64_t)(32 * NT2 * 16) > a->ws_bytes) return;
  pl.dp_tiles = (int)(q * G);
  pl.tail_s = (int)s;
  pl.tail_kt = (int)kt;
}

// row-slab kernel (64 < M <= ROWS_MAXM; k-contiguous A and B, batch 1, forward
// epilogues): whole-K 64-row tiles, 16 / 32 / 64 columns wide so the tiles cover >= 128 workgroups;
// 8 waves split K when it has >= 16 chunks (4 for GeGLU).  Taken where it measured faster than the
// 128-tile + split-K pair or the 256-tile kernel (tools/rows_bench.py, profiles/r03/rows_bench.log):
// K <= 2048 and <= 4096 output columns -- B = 1 SigLIP q|k|v 20.9 -> 12.0 us, o 14.6 -> 9.0 us, Gemma
// q|k|v / o at 276 rows 19.8 -> 18.1 us, action expert (320 rows) q|k|v 17.5 -> 11.0, o 16.0 -> 13.4,
// gate|up + GeGLU 32.9 -> 25.8 us; the long-K / wide ones (SigLIP fc1 / fc2, 4096-K down projections,
// the 32768-wide Gemma gate|up) stay on the tile kernels.  PZ_GEMM_ROWS=0: never; =1: any 64 < M <= ROWS_MAXM
// (A/B runs; read per call)
constexpr int64_t ROWS_MAXM = 1024;  // (C5's 768 / 789 prefill rows: 21.32 vs 21.52 ms at 512)

// row-slab tile sizing: 64-row tiles (32-row tiles, twice the workgroups, measured slower on every shape:
// rows_bench.log), 16 * tnb columns wide, tnb halved from tnb_max until the tiles cover >= 128 workgroups
int rows_tnb(int64_t M, int64_t ncols, int tnb_max) {
  int tnb = tnb_max;
  while (tnb > 1 && (M + 63) / 64 * ((ncols + 16 * tnb - 1) / (16 * tnb)) < 128) tnb /= 2;
  return tnb;
}
void rows_tiles(Plan& pl, int64_t M, int64_t ncols, int tnb) {
  pl.kind = PATH_ROWS;
  pl.rows_tnb = tnb;
  pl.rows_tmb = 4;
  pl.tiles_m = (M + 63) / 64;
  pl.tiles_n = (ncols + 16 * tnb - 1) / (16 * tnb);
}

bool plan_rows(Plan& pl, const pz_gemm_args* a, int64_t ncols) {
  const char* er = getenv("PZ_GEMM_ROWS");
  if ((er && er[0] == '0') || a->M <= 64 || a->M > ROWS_MAXM || !pl.akc || !pl.bkc || a->batch != 1 ||
      a->epilogue >= PZ_EPI_DGELU || a->norm_w)
    return false;
  if (!(er && er[0] == '1') && (a->K > 2048 || ncols > 4096)) return false;
  // e4m3 weights with bf16 rows (W8A16): 64-chunks of whole 16-code loads
  if (a->fp8_mode == 2 && (a->K % 64 != 0 || a->ldb % 16 != 0)) return false;
  pl.rows_f8 = a->fp8_mode == 2;
  int tnb = rows_tnb(a->M, ncols, pl.geglu ? 2 : 4);
  pl.rows_w = (a->K + 63) / 64 >= 16 && !pl.geglu ? 8 : 4;
  const char* ew = getenv("PZ_ROWS_W");  // A/B overrides (read per call): waves 4 | 8, column blocks
  if (ew && (atoi(ew) == 4 || atoi(ew) == 8)) pl.rows_w = atoi(ew);
  const char* et = getenv("PZ_ROWS_TNB");
  if (et && (atoi(et) == 1 || atoi(et) == 2 || (atoi(et) == 4 && !pl.geglu))) tnb = atoi(et);
  rows_tiles(pl, a->M, ncols, tnb);
  return true;
}

// tall-tile kernel (pz_gemm_tall.hip): 64 < M <= 1024 rows, k-contiguous A and B, batch 1, bf16 operands, forward
// epilogues: one 256- or 320-row tile covers up to 320 rows (the B = 1 prefill's 276 rows in ONE row tile instead of
// the 8-phase kernel's two 256-row tiles), 64 output columns per tile, K split over blockIdx.y until the grid
// reaches ~256 workgroups.  Taken by default where it measured faster (tools/tall_bench.py,
// profiles/r04/tall_bench.log, and inside the B = 1 chunk, profiles/r04/infer_trace_split.txt): <= 320 rows against
// the long-K narrow projections (Gemma down 276 x 2048 x 16384: 49.8 -> 44.8 us isolated, 54.5 -> 44.0 us in the
// chunk incl. the merge; SigLIP fc2 256 x 1152 x 4304: 18.7 -> 18.1 us).  Not the B = 1 GeGLU gate|up: 55.4 vs
// 57.9 us isolated (weights L2/MALL-warm over the repeats) but 65.2 vs 60.7 us in the chunk, where they stream
// cold from HBM; slower on the short-K / narrow shapes the row-slab kernel takes and at 788 rows (the 8-phase
// kernel's 256-row tiles are then mostly full).  PZ_GEMM_TALL=1: every eligible shape, 0: never (A/B runs)
bool plan_tall(Plan& pl, const pz_gemm_args* a, int64_t ncols) {
  const char* e = getenv("PZ_GEMM_TALL");
  if (e && e[0] == '0') return false;
  if (!(e && e[0] == '1') &&
      !(a->M <= 320 && pl.bkc && !pl.geglu && a->K >= 4300 && ncols <= 2048))
    return false;
  if (!pl.bkc || pl.geglu) return false;  // plain k-contiguous B only (pz_gemm_tall.hip)
  if (!pl.akc || a->batch != 1 || a->fp8_mode != 0 || a->norm_w || a->epilogue >= PZ_EPI_DGELU ||
      a->M <= 64 || a->M > 1024 || a->K % 8 != 0)
    return false;
  const int64_t t5 = (a->M + 319) / 320, t4 = (a->M + 255) / 256;
  pl.tall_mi = t5 * 320 <= t4 * 256 ? 5 : 4;
  pl.tiles_m = pl.tall_mi == 5 ? t5 : t4;
  pl.tiles_n = (ncols + 63) / 64;
  const int64_t bkt = 64;
  const int64_t nk = (a->K + bkt - 1) / bkt;
  const int64_t units = pl.tiles_m * pl.tiles_n;
  int64_t S = (256 + units - 1) / units;
  S = S < nk / 4 ? S : nk / 4;  // >= 4 K-tiles per split
  S = S < 16 ? S : 16;
  if (S >= 2) {
    const int64_t per = (nk + S - 1) / S;
    const int64_t Se = (nk + per - 1) / per;
    const int64_t ldw = (a->N + 3) / 4 * 4;
    if (Se >= 2 && a->workspace && PZ_ALIGNED(a->workspace, 16) && Se * a->M * ldw * 4 <= a->ws_bytes) {
      pl.splits = (int)Se;
      pl.ksplit = per * bkt;
      pl.ldw = ldw;
    }
  }
  pl.kind = PATH_TALL;
  return true;
}

// skinny-64 split-K combined in the launch: S tile-private [64][nc] fp32 slabs per tile fit the workspace (bf16 C,
// forward epilogue)
static bool sk64_fits(const Plan& pl, const pz_gemm_args* a) {
  return (int64_t)pl.splits * pl.tiles_n * 64 * pl.skinny_nc * 4 <= a->ws_bytes && !a->c_fp32 &&
         a->epilogue < PZ_EPI_DGELU;
}

constexpr int64_t MIN_UNITS_256 = 160;  // workgroups the 256-tile path must reach to be taken

// the kernel, its tiles and its split for a validated argument set (make_plan adds what follows from them)
Plan route(const pz_gemm_args* a) {
  Plan pl{};
  pl.akc = a->a_kcontig != 0;
  pl.bkc = a->b_kcontig != 0;
  pl.geglu = a->epilogue == PZ_EPI_GEGLU;
  pl.x = a->K2 > 0;
  pl.fp8 = a->fp8_mode;
  pl.batch = a->batch;
  const int64_t ncols = pl.geglu ? a->geglu_inter : a->N;
  // rank extension (K2 > 0): only the 8-phase kernel (whole tiles, A k-contiguous, K % 8 == 0, the usual row /
  // column / workgroup thresholds) and the 128-tile kernel (whole K) carry it; every other path is skipped
  if (a->K2 > 0) {
    const int64_t cwx = pl.geglu ? BT / 2 : BT;
    const int64_t tm = (a->M + BT - 1) / BT, tn = (ncols + cwx - 1) / cwx;
    if (pl.akc && a->K % 8 == 0 && a->M >= 512 && ncols >= (pl.geglu ? 256 : 512) && tm * tn >= 160) {
      pl.kind = PATH_256;
      pl.tiles_m = tm;
      pl.tiles_n = tn;
      return pl;
    }
    pl.kind = PATH_TILE;
    pl.tiles_m = (a->M + BM - 1) / BM;
    pl.tiles_n = (ncols + (pl.geglu ? BN / 2 : BN) - 1) / (pl.geglu ? BN / 2 : BN);
    pl.wm = pl.geglu ? 4 : 2;
    return pl;
  }
  // fp8 W8A8: the 8-phase 256-tile kernel on code pairs (K, lda, ldb halved by the caller of make_plan); the row-slab
  // shapes (64 < M <= 1024, <= 2048 codes of K in 128-code chunks, <= 4096 columns, no GeGLU: C5's prefill q|k|v / o)
  // take the W8A8 row-slab kernel
  if (a->fp8_mode == 1) {
    if (!pl.geglu && a->M > 64 && a->M <= 1024 && a->K % 64 == 0 && a->K <= 1024 &&
        ncols <= 4096 && a->a_row_scale) {
      pl.rows_f8 = 2;
      pl.rows_w = a->K / 64 >= 8 ? 8 : 4;
      rows_tiles(pl, a->M, ncols, rows_tnb(a->M, ncols, 4));
      return pl;
    }
    pl.kind = PATH_256;
    pl.tiles_m = (a->M + BT - 1) / BT;
    pl.tiles_n = (ncols + (pl.geglu ? BT / 2 : BT) - 1) / (pl.geglu ? BT / 2 : BT);
    plan_tail(pl, a);
    return pl;
  }
  // skinny-64 path: 16 < M <= 64 rows (bf16), or any M <= 64 with fp8 weights (W8A16)
  const bool sk64_ok = a->M <= 64 && pl.akc && pl.bkc && a->K % 64 == 0 && a->batch == 1 &&
                       !a->c_fp32 && a->epilogue < PZ_EPI_DGELU;
  if (a->fp8_mode == 2 && a->M > 64) {  // W8A16 above 64 rows: the row-slab kernel or nothing (pz_gemm rejects)
    if (!plan_rows(pl, a, ncols)) pl.kind = PATH_NONE;
    return pl;
  }
  if (a->fp8_mode == 2 || (sk64_ok && a->M > 16)) {
    pl.kind = PATH_SKINNY64;
    pl.skinny_mb = (int)((a->M + 15) / 16);
    pl.skinny_mb = pl.skinny_mb == 3 ? 4 : pl.skinny_mb;
    // 16 real columns per block, 8 waves: every block re-reads the (L2-resident) activation rows, so
    // narrower blocks multiply that traffic -- measured at 50 rows (tools/skinny_bench.py): q|k|v
    // 7.3 vs 16.8 us, gate|up 8.6 vs 25.6 us for 16 vs 4 columns; W = 8 never slower than 4
    pl.skinny_w = a->K / 64 >= 8 ? 8 : 4;
    pl.skinny_nc = 16;
    // narrow outputs (o / down projections: 64 blocks of 16 columns) split K over blockIdx.z so the
    // weight stream spreads over ~256 workgroups; partials summed in the launch or by splitk_epilogue_kernel
    // (no fused norm / GeGLU with a split)
    {
      const int64_t nblk = (ncols + 15) / 16;
      const int64_t kch = a->K / 64;
      if (!a->norm_w && !pl.geglu && a->workspace && nblk < 128 &&
          kch >= 16) {
        int64_t S = (256 + nblk - 1) / nblk;
        S = S < kch / 8 ? S : kch / 8;
        S = S < 8 ? S : 8;
        const int64_t ldw = (a->N + 3) / 4 * 4;
        if (S >= 2 && S * a->M * ldw * 4 <= a->ws_bytes && PZ_ALIGNED(a->workspace, 16)) {
          const int64_t per = (kch + S - 1) / S;
          pl.splits = (int)((kch + per - 1) / per);
          pl.ksplit = per * 64;
          pl.ldw = ldw;
        }
      }
    }
    pl.tiles_n = (ncols + pl.skinny_nc - 1) / pl.skinny_nc;
    return pl;
  }
  // GEMV path (M <= 8, K % 512 == 0: the B = 1..2 denoise rows): every CU streams its weight slice
  // (pz_gemv.hip); PZ_GEMV=0 falls back to the MFMA skinny kernel below
  if (pz_gemv_supported(a)) {
    pl.kind = PATH_GEMV;
    pl.gemv_mr = a->M <= 4 ? 4 : 8;
    return pl;
  }
  // skinny path: few rows, weights streamed once (inference denoise / proprio rows)
  if (a->M <= 16 && pl.akc && pl.bkc && a->K % 32 == 0 && !a->c_fp32 && a->epilogue < PZ_EPI_DGELU) {
    const int64_t kch = a->K / 32;
    pl.kind = PATH_SKINNY;
    pl.skinny_w = kch >= 64 ? 16 : (kch >= 32 ? 8 : 4);
    // PZ_SKINNY_MINNC=8|4: fewer columns per block for narrow outputs until the blocks cover the CUs
    // (A/B runs; measured slower at B=1 -- 9.9 vs 8.8 us for the 1024-wide o/down projections -- so
    // every block takes 16 columns by default)
    const char* e = getenv("PZ_SKINNY_MINNC");
    const int min_nc = e ? atoi(e) : 16;
    pl.skinny_nc = 16;
    while (pl.skinny_nc > 4 && pl.skinny_nc / 2 >= min_nc &&
           a->batch * ((ncols + pl.skinny_nc - 1) / pl.skinny_nc) < pz_device_cus())
      pl.skinny_nc /= 2;
    pl.tiles_n = (ncols + pl.skinny_nc - 1) / pl.skinny_nc;
    return pl;
  }
  const int64_t cw = pl.geglu ? BT / 2 : BT;
  if (plan_tall(pl, a, ncols)) return pl;
  // the row-slab kernel before the 256-tile kernels (action-expert gate|up at 320 rows); PZ_ROWS_FIRST=1 for
  // every shape it takes (A/B runs; read per call)
  {
    const char* ef = getenv("PZ_ROWS_FIRST");
    if ((pl.geglu || (ef && ef[0] == '1')) && plan_rows(pl, a, ncols)) return pl;
  }
  // rows from which the 256-tile kernels are tried: 256 for the GeGLU GEMM and long-K GEMMs (prefill
  // at B=1, 276 rows: 64 vs 78 us and 51 vs 56 us measured), 512 otherwise (narrow prefill GEMMs
  // are faster on 128-row tiles)
  const int64_t min_m = (pl.geglu || a->K >= 8192 || (a->batch > 1 && !pl.akc && !pl.bkc)) ? 256 : 512;
  // at most half a round of 256-tiles at short K (the action expert's 1024- and 1280-row GEMMs at micro-batch 256): the 128-tile
  // kernel (+ split-K) beats the 256-tile split tail, 22-37 vs 29-45 us per launch, except at K 8192
  // (profiles/r05/attn_gemm_ab.log)
  const bool small_short = !pl.geglu && a->batch == 1 && a->M >= 1024 && a->K <= 4096 &&
                           ((a->M + BT - 1) / BT) * ((ncols + cw - 1) / cw) <= 128;
  // batched TN GEMMs with >= 256 x 256 outputs per batch entry (the joint attention's dK = dS^T Q and dV = P^T dO,
  // 288 x 256 per sample): the 256-tile kernel, two row tiles per sample, 173 vs 190-203 us (dV of the 5-row action
  // mixture 28.7 vs 40.6 us) against the 128-tile kernel (profiles/r05/attn_gemm_ab_r5s.log)
  const bool batched_tn = a->batch > 1 && !pl.akc && !pl.bkc && a->M >= 256 && ncols >= 256;
  const int64_t min_n = pl.geglu || batched_tn ? 256 : 512;  // output columns from which the 256-tile path is tried
  if (a->K % 8 == 0 && a->M >= min_m && ncols >= min_n && !small_short) {
    const int64_t tm = (a->M + BT - 1) / BT, tn = (ncols + cw - 1) / cw;
    Plan cand = pl;
    cand.kind = PATH_256;
    cand.tiles_m = tm;
    cand.tiles_n = tn;
    plan_tail(cand, a);
    // enough workgroups to fill the chip: whole tiles, or tiles split into K-pieces
    const int64_t units = cand.tail_s ? cand.dp_tiles + (tm * tn - cand.dp_tiles) * cand.tail_s : a->batch * tm * tn;
    if (units >= MIN_UNITS_256) return cand;
  }
  if (plan_rows(pl, a, ncols)) return pl;
  pl.kind = PATH_TILE;
  pl.tiles_m = (a->M + BM - 1) / BM;
  pl.tiles_n = (ncols + (pl.geglu ? BN / 2 : BN) - 1) / (pl.geglu ? BN / 2 : BN);
  pl.wm = pl.geglu ? 4 : 2;
  pl.tag = (pl.geglu && pl.akc && a->M >= 2048) ? 1 : 0;
  // split-K when one 128x128 tile per WG leaves most of the 256 CUs idle
  const int64_t tiles = pl.tiles_m * pl.tiles_n;
  const int64_t nk = (a->K + BK - 1) / BK;
  if (a->batch == 1 && a->workspace && tiles < 120 && nk >= 4) {
    int64_t S = (240 + tiles - 1) / tiles;
    S = S < 16 ? S : 16;
    S = S < nk / 2 ? S : nk / 2;
    if (S >= 2) {
      const int64_t ks = ((nk + S - 1) / S) * BK;
      const int64_t Se = (a->K + ks - 1) / ks;
      const int64_t ldw = pl.geglu ? 2 * a->geglu_inter : (a->N + 3) / 4 * 4;
      if (Se >= 2 && Se * a->M * ldw * 4 <= a->ws_bytes && PZ_ALIGNED(a->workspace, 16)) {
        pl.kind = PATH_SPLIT;
        pl.splits = (int)Se;
        pl.ksplit = ks;
        pl.ldw = ldw;
      }
    }
  }
  return pl;
}

// The whole plan for a validated argument set: pz_gemm launches it, pz_gemm_kernel_name prints it.
// group > 0: that tile order (the RoPE GEMMs keep 8); 0: by shape or PZ_GEMM_GROUP.
Plan make_plan(const pz_gemm_args* a, int group = 0) {
  Plan pl = route(a);
  const int64_t T = pl.tiles_m * pl.tiles_n;
  if (pl.kind == PATH_256) {
    pl.khalf = use_khalf(pl.akc, pl.bkc, a->M, a->N, a->K);
    pl.ktail = a->K % 64 != 0;
    pl.units = (int)(pl.tail_s ? pl.dp_tiles + (T - pl.dp_tiles) * pl.tail_s : T);
  }
  // 8-phase tile order (tile_coords): super-rows of 2 row tiles instead of 8 for the narrow long-K GEMMs (<= 8
  // column tiles, K >= 16384: the Gemma gate|up dgrad, down forward, down / gate|up wgrads) and the DGEGLU dgrad --
  // measured per shape at micro-batch 256 (profiles/r06/gemm_group_ab.txt: gate|up dgrad 125.8 -> 121.4 ms,
  // DGEGLU 83.7 -> 81.5, down fwd 62.2 -> 61.2, wgrad 127.9 -> 127.0); the GeGLU forward keeps 8 (139.9 vs 142.2).
  // PZ_GEMM_GROUP overrides (A/B; read per call).
  pl.group = group;
  if (group <= 0) {
    const char* e = getenv("PZ_GEMM_GROUP");
    if (e && atoi(e) >= 1 && atoi(e) <= 64) pl.group = atoi(e);
    else pl.group = (a->K >= 16384 && pl.tiles_n <= 8) || a->epilogue == PZ_EPI_DGEGLU ? 2 : 8;
  }
  // batched 128-tile launches: the XCD-grouped 1-D grid (PZ_GEMM_BATCH_XCD=0: the 2-D grid; A/B, read once)
  static const bool xb = [] {
    const char* e = getenv("PZ_GEMM_BATCH_XCD");
    return !(e && e[0] == '0');
  }();
  pl.batch_xcd = xb && pl.kind == PATH_TILE && a->batch >= 8 && a->batch % 8 == 0 && T * a->batch < (1LL << 31);
  // skinny-64 split-K (2..8 slices over < 128 column blocks): summed in the launch unless PZ_SK64_FUSED=0 (the
  // two-launch form, A/B; read per call) or the tile-private slabs do not fit
  pl.sk_fused = pl.kind == PATH_SKINNY64 && pl.ksplit > 0 && pl.splits > 1 && pl.splits <= 8 && pl.tiles_n <= 256 &&
                sk64_fits(pl, a) && !sk64_two_launch();
  return pl;
}

// fp8 W8A8: the planner and the kernels see K / lda / ldb in code pairs (a8: the halved copy)
const pz_gemm_args* code_pairs(const pz_gemm_args* a, pz_gemm_args& a8) {
  if (a->fp8_mode != 1) return a;
  a8 = *a;
  a8.K = a->K / 2;
  a8.lda = a->lda / 2;
  a8.ldb = a->ldb / 2;
  return &a8;
}

// the kernels' argument block: operands, strides and epilogue of a, tiles / split / tail / tile order of its plan
GemmP gemm_params(const pz_gemm_args* a, const Plan& pl) {
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.A = (const bf16_t*)a->A;
  p.B = (const bf16_t*)a->B;
  p.C = a->C;
  p.bias = (const bf16_t*)a->bias;
  p.resid = (const bf16_t*)a->resid;
  p.aux = (bf16_t*)a->aux;
  p.M = a->M; p.N = a->N; p.K = a->K;
  p.lda = a->lda; p.ldb = a->ldb; p.ldc = a->ldc;
  p.ld_resid = a->ld_resid; p.ld_aux = a->ld_aux; p.geglu_I = a->geglu_inter;
  p.batch_inner = a->batch_inner;
  p.sAo = a->sA_outer; p.sAi = a->sA_inner;
  p.sBo = a->sB_outer; p.sBi = a->sB_inner;
  p.sCo = a->sC_outer; p.sCi = a->sC_inner;
  p.sRo = a->sR_outer; p.sRi = a->sR_inner;
  p.epi = a->epilogue;
  p.c_fp32 = a->c_fp32;
  p.beta = a->beta_accum;
  p.alpha = a->alpha;
  p.nw = (const bf16_t*)a->norm_w;
  p.neps = a->norm_eps;
  p.rs = a->fp8_mode == 1 ? a->a_row_scale : nullptr;
  if (a->K2 > 0) {
    p.A2 = (const bf16_t*)a->A2;
    p.B2 = (const bf16_t*)a->B2;
    p.lda2 = a->lda2; p.ldb2 = a->ldb2; p.K2 = a->K2;
  }
  p.tiles_m = (int)pl.tiles_m;
  p.tiles_n = (int)pl.tiles_n;
  p.group = pl.group;
  p.batch_xcd = pl.batch_xcd ? (int)pl.batch : 0;
  if (pl.ksplit > 0 || pl.tail_s) p.ws = (float*)a->workspace;
  p.ksplit = pl.ksplit;
  p.ldw = pl.ldw;
  p.dp_tiles = pl.dp_tiles;
  p.tail_s = pl.tail_s;
  p.tail_kt = pl.tail_kt;
  return p;
}

const char* bstr(bool b) { return b ? "true" : "false"; }
}  // namespace

extern "C" const char* pz_gemm_kernel_name(const pz_gemm_args* a) {
  static thread_local char buf[160];
  if (!a) return "";
  pz_gemm_args a8;
  const Plan pl = make_plan(code_pairs(a, a8));
  const char* k8 = pl.khalf ? "gemm8k_kernel" : "gemm8p_kernel";
  switch (pl.kind) {
    case PATH_SKINNY:
      snprintf(buf, sizeof(buf), "gemm_skinny_kernel<%d, %d>", pl.skinny_w, pl.skinny_nc);
      break;
    case PATH_SKINNY64:
      snprintf(buf, sizeof(buf), "gemm_skinny64_kernel<%d, %d, %d, %s>%s", pl.skinny_w, pl.skinny_nc, pl.skinny_mb,
               bstr(pl.fp8 == 2), pl.ksplit > 0 && !pl.sk_fused ? "+splitk_epilogue_kernel" : "");
      break;
    case PATH_NONE:  // (printed as the skinny-64 plan it once was left as: the routing fixture holds the string)
      snprintf(buf, sizeof(buf), "gemm_skinny64_kernel<0, 0, 0, true>");
      break;
    case PATH_GEMV:
      snprintf(buf, sizeof(buf), "gemv_kernel<M<=%d>", pl.gemv_mr);
      break;
    case PATH_256:
      if (pl.x)
        snprintf(buf, sizeof(buf), "gemm8p_x_kernel<%s, %s, %s>", bstr(pl.akc), bstr(pl.bkc), bstr(pl.geglu));
      else if (pl.tail_s)
        snprintf(buf, sizeof(buf), "%s<%s, %s, %s, %s>+gemm8p_tail_epilogue(tail %lld x %d)", k8, bstr(pl.akc),
                 bstr(pl.bkc), bstr(pl.geglu), bstr(pl.ktail), (long long)(pl.tiles_m * pl.tiles_n - pl.dp_tiles),
                 pl.tail_s);
      else
        snprintf(buf, sizeof(buf), "%s<%s, %s, %s, %s>", k8, bstr(pl.akc), bstr(pl.bkc), bstr(pl.geglu),
                 bstr(pl.ktail));
      break;
    case PATH_TILE:
      if (pl.x) snprintf(buf, sizeof(buf), "gemm_x_kernel<%s, %s, %d>", bstr(pl.akc), bstr(pl.bkc), pl.wm);
      else snprintf(buf, sizeof(buf), "gemm_kernel<%s, %s, %d, %d>", bstr(pl.akc), bstr(pl.bkc), pl.wm, pl.tag);
      break;
    case PATH_ROWS:
      if (pl.rows_f8 == 2)
        snprintf(buf, sizeof(buf), "gemm_rows_f8a_kernel<%d, %d, %d>", pl.rows_w, pl.rows_tmb, pl.rows_tnb);
      else
        snprintf(buf, sizeof(buf), "gemm_rows_kernel<%d, %d, %d, %s, %s>", pl.rows_w, pl.rows_tmb, pl.rows_tnb,
                 bstr(pl.geglu), bstr(pl.rows_f8 == 1));
      break;
    case PATH_TALL:  // (the label keeps the two flags of the retired GeGLU / k-strided-B forms: profile logs key on it)
      snprintf(buf, sizeof(buf), "gemm_tall_kernel<%d, 2, 64, 3, false, true>%s", pl.tall_mi,
               pl.splits > 1 ? "+splitk_epilogue_kernel" : "");
      break;
    case PATH_SPLIT:
      snprintf(buf, sizeof(buf), "gemm_kernel<%s, %s, %d, %d>+splitk_epilogue_kernel(S=%d)", bstr(pl.akc),
               bstr(pl.bkc), pl.wm, pl.tag, pl.splits);
      break;
  }
  return buf;
}

extern "C" int pz_gemm(const pz_gemm_args* a, void* stream) {
  PZ_CHECK_ARG(a != nullptr, "pz_gemm: null args");
  PZ_CHECK_ARG(a->M > 0 && a->N > 0 && a->K > 0, "pz_gemm: bad dims M=%lld N=%lld K=%lld",
               (long long)a->M, (long long)a->N, (long long)a->K);
  PZ_CHECK_ARG(a->A && a->B && a->C, "pz_gemm: null operand");
  PZ_CHECK_ARG(a->batch >= 1 && a->batch_inner >= 1 && a->batch % a->batch_inner == 0,
               "pz_gemm: bad batch %lld/%lld", (long long)a->batch, (long long)a->batch_inner);
  PZ_CHECK_ARG(PZ_ALIGNED(a->A, 16) && PZ_ALIGNED(a->B, 16), "pz_gemm: A/B must be 16-byte aligned");
  PZ_CHECK_ARG(a->lda % 8 == 0 && a->ldb % 8 == 0, "pz_gemm: lda/ldb must be multiples of 8");
  PZ_CHECK_ARG(a->ldc % 4 == 0 && PZ_ALIGNED(a->C, 8), "pz_gemm: ldc %% 4 and C 8-byte alignment");
  PZ_CHECK_ARG(a->sA_outer % 8 == 0 && a->sA_inner % 8 == 0 && a->sB_outer % 8 == 0 &&
                   a->sB_inner % 8 == 0 && a->sC_outer % 4 == 0 && a->sC_inner % 4 == 0,
               "pz_gemm: batch strides must keep 16-byte alignment");
  if (a->a_kcontig) PZ_CHECK_ARG(a->K % 8 == 0, "pz_gemm: k-contiguous A needs K %% 8 == 0");
  else PZ_CHECK_ARG(a->M % 8 == 0, "pz_gemm: k-strided A needs M %% 8 == 0");
  if (a->b_kcontig) PZ_CHECK_ARG(a->K % 8 == 0, "pz_gemm: k-contiguous B needs K %% 8 == 0");
  else PZ_CHECK_ARG(a->N % 8 == 0, "pz_gemm: k-strided B needs N %% 8 == 0");
  const bool geglu = a->epilogue == PZ_EPI_GEGLU;
  if (geglu) {
    PZ_CHECK_ARG(a->b_kcontig && a->geglu_inter > 0 && a->N == 2 * a->geglu_inter && a->batch == 1 &&
                     !a->beta_accum && !a->resid && !a->bias && !a->c_fp32 && a->geglu_inter % 4 == 0,
                 "pz_gemm: GEGLU needs k-contiguous B = [gate; up] (N = 2I), no batch/bias/resid");
  }
  if (a->epilogue == PZ_EPI_GELU || a->epilogue == PZ_EPI_SILU)
    PZ_CHECK_ARG(a->batch == 1, "pz_gemm: activation epilogue is unbatched");
  PZ_CHECK_ARG(a->epilogue >= PZ_EPI_NONE && a->epilogue <= PZ_EPI_DGEGLU, "pz_gemm: unknown epilogue %d",
               (int)a->epilogue);
  PZ_CHECK_ARG(!(a->c_fp32 && a->beta_accum && a->resid), "pz_gemm: fp32 beta accumulation takes no resid");
  if (a->epilogue >= PZ_EPI_DGELU) {
    PZ_CHECK_ARG(a->batch == 1 && a->aux && !a->bias && !a->resid && !a->beta_accum && !a->c_fp32,
                 "pz_gemm: backward epilogues read aux, write bf16 C, unbatched, no bias/resid/beta");
    if (a->epilogue == PZ_EPI_DGEGLU)
      PZ_CHECK_ARG(a->geglu_inter == a->N && a->ldc >= 2 * a->N && a->ld_aux >= 2 * a->N,
                   "pz_gemm: DGEGLU needs N == geglu_inter and [*, 2I] aux / C rows");
  }
  if (a->aux) PZ_CHECK_ARG(a->ld_aux % 4 == 0 && PZ_ALIGNED(a->aux, 8), "pz_gemm: aux alignment");
  PZ_CHECK_ARG(a->ws_bytes >= 0, "pz_gemm: negative ws_bytes");
  PZ_CHECK_ARG(a->fp8_mode >= 0 && a->fp8_mode <= 2, "pz_gemm: fp8_mode %d", (int)a->fp8_mode);
  PZ_CHECK_ARG(a->K2 >= 0, "pz_gemm: negative K2");
  if (a->K2 > 0) {
    if (a->fp8_mode != 0) {
      pz_set_error("pz_gemm: the rank extension (K2 > 0) takes bf16 operands only");
      return PZ_ERR_UNSUPPORTED;
    }
    PZ_CHECK_ARG(a->K2 % 8 == 0 && a->K2 >= 8 && a->K2 <= 384, "pz_gemm: K2 = %lld must be a multiple of 8 in [8, 384]",
                 (long long)a->K2);
    PZ_CHECK_ARG(a->A2 && a->B2 && PZ_ALIGNED(a->A2, 16) && PZ_ALIGNED(a->B2, 16) && a->lda2 % 8 == 0 &&
                     a->ldb2 % 8 == 0,
                 "pz_gemm: A2 / B2 must be 16-byte aligned with lda2 / ldb2 %% 8 == 0");
    PZ_CHECK_ARG(a->batch == 1 && !a->norm_w, "pz_gemm: the rank extension is unbatched and takes no fused norm");
  }
  if (a->fp8_mode == 1)
    PZ_CHECK_ARG(a->a_kcontig && a->b_kcontig && a->batch == 1 && !a->norm_w && a->epilogue <= PZ_EPI_SILU &&
                     a->K % 16 == 0 && a->lda % 16 == 0 && a->ldb % 16 == 0,
                 "pz_gemm: fp8 W8A8 needs k-contiguous A [M][K] and B [N][K] codes, batch 1, K / lda / ldb "
                 "%% 16 == 0, a forward epilogue and no fused norm");
  if (a->fp8_mode == 2)
    PZ_CHECK_ARG(a->a_kcontig && a->b_kcontig && a->batch == 1 && a->K % 64 == 0 && !a->c_fp32 &&
                     a->epilogue < PZ_EPI_DGELU && a->ldb % 16 == 0,
                 "pz_gemm: fp8 weights with bf16 rows (W8A16) need k-contiguous A and B, batch 1, "
                 "K %% 64 == 0, ldb %% 16 == 0, bf16 C and a forward epilogue");
  pz_gemm_args a8;
  a = code_pairs(a, a8);

  const Plan pl = make_plan(a);
  PZ_CHECK_ARG(pl.kind != PATH_NONE,
               "pz_gemm: W8A16 above 64 rows needs a row-slab shape (M <= 1024, K <= 2048, <= 4096 columns)");
  if (a->norm_w)
    PZ_CHECK_ARG((pl.kind == PATH_GEMV || pl.kind == PATH_SKINNY || pl.kind == PATH_SKINNY64) &&
                     PZ_ALIGNED(a->norm_w, 16),
                 "pz_gemm: fused RMSNorm needs the few-row paths (M <= 64, k-contiguous A/B, K %% 32 == 0 "
                 "(M <= 16) or K %% 64 == 0) and a 16-byte aligned weight");
  if (pl.kind == PATH_SKINNY) PZ_CHECK_ARG(a->batch < 65536, "pz_gemm: batch too large");
  PZ_CHECK_ARG(pl.tiles_m * pl.tiles_n < (1LL << 31) && a->batch < 65536, "pz_gemm: grid too large");
  const GemmP p = gemm_params(a, pl);
  hipStream_t st = (hipStream_t)stream;
  switch (pl.kind) {
    case PATH_GEMV: return pz_gemv_launch(a, pl.gemv_mr, st);
    case PATH_SKINNY: return pz_skinny_launch(p, pl, st);
    case PATH_SKINNY64: return pz_sk64_launch(p, pl, st);
    case PATH_ROWS: return pz_rows_launch(p, pl, st);
    case PATH_TALL: return pz_tall_launch(p, pl, st);
    case PATH_256: return pz_8p_launch(p, pl, st);
    case PATH_TILE:
    case PATH_SPLIT: return pz_tile_launch(p, pl, st);
    case PATH_NONE: break;
  }
  return PZ_ERR_INVALID_ARG;
}

// q|k|v projection + RoPE + joint Q / K / V scatter in one 8-phase GEMM launch (training / prefill rows:
// mixture.py:162-215 + utils.py:4-16 + joint_model.py:170-257).  PZ_ERR_UNSUPPORTED (no error text) when the
// shape does not take the 8-phase 256-tile kernel: the caller then runs pz_gemm + pz_qkv_rope_split.
extern "C" int pz_gemm_qkv_rope(const pz_qkv_rope_args* a, void* stream) {
  PZ_CHECK_ARG(a && a->x && a->W && a->pos && a->cs && a->k_out && a->v_out && a->M > 0 && a->K > 0,
               "gemm_qkv_rope: bad args");
  PZ_CHECK_ARG(a->nh >= 1 && a->N == (a->nh + 2) * a->hd && a->T > 0 && a->M % a->T == 0,
               "gemm_qkv_rope: N = (nh + 2) * hd, M %% T == 0");
  // head_dim 256 (one 256-column 8-phase tile / 16 skinny blocks per head) and Q written: otherwise not this
  // kernel (no error text)
  if (a->hd != BT || !a->q_out) return PZ_ERR_UNSUPPORTED;
  PZ_CHECK_ARG(PZ_ALIGNED(a->x, 16) && PZ_ALIGNED(a->W, 16) && a->ldx % 8 == 0 && a->ldw % 8 == 0 && a->K % 8 == 0 &&
                   PZ_ALIGNED(a->q_out, 16) && PZ_ALIGNED(a->k_out, 16) && PZ_ALIGNED(a->v_out, 16),
               "gemm_qkv_rope: 16-byte alignment");
  pz_gemm_args g;
  memset(&g, 0, sizeof(g));
  g.M = a->M; g.N = a->N; g.K = a->K;
  g.A = a->x; g.lda = a->ldx; g.a_kcontig = 1;
  g.B = a->W; g.ldb = a->ldw; g.b_kcontig = 1;
  g.C = a->q_out; g.ldc = a->N;
  g.batch = 1; g.batch_inner = 1;
  g.alpha = 1.f;
  g.norm_w = a->norm_w;
  g.norm_eps = a->norm_eps;
  if (a->K2 > 0) {
    if (a->w_fp8 || a->norm_w) return PZ_ERR_UNSUPPORTED;
    PZ_CHECK_ARG(a->K2 % 8 == 0 && a->K2 >= 8 && a->K2 <= 384 && a->x2 && a->W2 && PZ_ALIGNED(a->x2, 16) &&
                     PZ_ALIGNED(a->W2, 16) && a->ldx2 % 8 == 0 && a->ldw2 % 8 == 0,
                 "gemm_qkv_rope: rank extension needs K2 %% 8 == 0 in [8, 384], 16-byte aligned x2 / W2");
    g.A2 = a->x2; g.lda2 = a->ldx2;
    g.B2 = a->W2; g.ldb2 = a->ldw2;
    g.K2 = a->K2;
  }
  if (a->w_fp8) {
    PZ_CHECK_ARG(a->ldw % 16 == 0, "gemm_qkv_rope: fp8 weights need ldw %% 16 == 0");
    g.fp8_mode = 2;
    g.alpha = a->w_scale;
  }
  // no workspace: whole tiles only (the tail merge has no RoPE epilogue); tile order 8, whatever PZ_GEMM_GROUP says
  const Plan pl = make_plan(&g, 8);
  GemmP p = gemm_params(&g, pl);
  p.rpos = a->pos;
  p.rcs = a->cs;
  p.rq = (bf16_t*)a->q_out;
  p.rk = (bf16_t*)a->k_out;
  p.rv = (bf16_t*)a->v_out;
  p.rT = a->T; p.rnh = a->nh; p.rLq = a->Lq; p.rqoff = a->qoff; p.rLk = a->Lk; p.rkoff = a->koff;
  // few rows (16 < M <= 64: C5's 50-row denoise chunk): the skinny-64 kernel with the RoPE epilogue, the
  // Gemma RMSNorm optionally fused (mixture.py:162-215 + utils.py:4-16 in one launch)
  if (pl.kind == PATH_SKINNY64 && pl.ksplit == 0 && a->K % 64 == 0 && a->N % 256 == 0 && a->M <= 64 &&
      (!a->norm_w || PZ_ALIGNED(a->norm_w, 16)))
    return pz_sk64_launch(p, pl, (hipStream_t)stream);
  if (a->norm_w || a->w_fp8 || pl.kind != PATH_256) return PZ_ERR_UNSUPPORTED;
  return pz_8p_launch(p, pl, (hipStream_t)stream);
}
