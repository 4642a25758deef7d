// gemm.hip -- dispatch of the GEMM family: cmda_gemm = validate, plan (plan_gemm: tile / split-K heuristics, kernel family, stages),
// run the plan.  Kernel templates and their documentation: gemm_kernels.h; the instantiations live in gemm_t0..t3.hip (LDS-DMA
// tiles), gemm_reg*.hip (register-staged) and the kernels' own files (gemm_pp / wg / lean / x3 / x3_lean.hip).
#include "gemm_kernels.h"

namespace {

// The LDS-DMA kernels' 4-stage latency configuration (four-wave tiles; the general and the lean kernel alike): the whole grid is resident
// at once even at 4 stages (64x64: 64 KiB -> 2 blocks per CU; the wider tiles: 96 / 128 KiB -> 1 block per CU) and every block runs
// >= 12 k-tiles (K >= 768).  12: in the step 77.5-78.1 ms against 78.0-78.2 at 3 and 78.2-79.2 at 40; deeper than 4 stages -- 8 x 16 KiB
// on the 64x64 tile, 6 x 24 KiB on 128x64, one block per CU -- measured slower on every shape of the step (profiles/r02_gemm_sweep.txt)
int plan_stages(const GemmHint& h, GemmTile tile, long blocks, long nkt) {
  if (tile == kTile256x256) return 2;
  if (h.stages) return h.stages == 4 ? 4 : 2;
  return blocks <= 256L * (tile == kTile64x64 ? 2 : 1) && nkt >= 12 ? 4 : 2;
}

// Pure: dereferences no operand pointer, launches nothing.  `p`: validated (cmda_gemm), batch2 >= 1.
GemmPlan plan_gemm(const GemmParams& p) {
  GemmPlan plan{CMDA_ERR_UNSUPPORTED, kGemmNone, kTile64x64, 0, 4, p.splits, false};
  const GemmHint h = decode_hint(p.tile_hint);
  if (!h.valid) return plan;   // a tuning script must not believe it switched something
  plan.general_addr = h.general_addr;
  const bool bf16 = p.dtype == CMDA_BF16;   // (fp32 storage, exact or split-bf16: same tile heuristics)
  // Tile / split-K choice.  256 CUs want >= ~2 blocks each; never waste half a tile on N <= 64.
  const long zb = (long)p.batch * p.batch2;
  auto blocks = [&](GemmTile t) { return (long)((p.M + kGemmTileBM[t] - 1) / kGemmTileBM[t]) * ((p.N + kGemmTileBN[t] - 1) / kGemmTileBN[t]) * zb; };
  const int BK = bf16 ? 64 : 32;
  const int nkt = (p.K + BK - 1) / BK;
  GemmTile tile;
  if (p.atomic && p.splits <= 0) {
    // accumulate-by-atomics GEMMs (weight gradients): few output tiles, very long contraction -> largest tile that
    // fits the output, then split K until the grid fills the chip
    // Every split adds one fp32 atomic per output element (chip-wide ~1.3 TB/s), so splits stay small and the tile
    // only grows to 128x128 when the output alone already has enough tiles.
    tile = kTile64x64;
    if (p.M > 64 && p.N > 64) {
      // 256x256: gemm_wg.hip (32x32x16 MFMA; both operands stream from beyond L2, so the tile size is the speed: the head's pointwise
      // weight gradients 256 x 1024 over 262144 pixels are 4 tiles x 61 splits, its 3x3 bottleneck 36 tiles x 7 splits)
      if (bf16 && p.M >= 256 && p.N >= 256 && p.A.conv != 1 && (blocks(kTile256x256) >= 32 || (blocks(kTile256x256) >= 4 && nkt >= 1024)))
        tile = kTile256x256;
      else if (blocks(kTile128x128) >= 64 || (blocks(kTile128x128) >= 16 && nkt >= 1024)) tile = kTile128x128;  // very deep K: split further
      else if (blocks(kTile128x64) >= 48 && nkt >= 256) tile = kTile128x64;  // e.g. the 320x1280 MixFFN weight gradients at K >= 16 k rows (57 vs 72 us on
                                                                             // 64x64 tiles); at the UDA step's K = 8192 the 64x64 tile is ahead (30.0 vs 32.5 us)
    }
    const long b = blocks(tile);
    // im2col weight gradients (very deep K, output of a few MB): let the wave-quantisation search below look twice as far
    long s = ((p.B.conv == 1 ? 1024 : 512) + b - 1) / b;
    s = std::min<long>(s, std::max(1, nkt / 8));
    const long out_bytes = (long)p.M * p.N * 4 * zb;
    s = std::min<long>(s, std::max<long>(16, (32L << 20) / std::max<long>(out_bytes, 1)));  // atomic traffic bound
    if (tile == kTile256x256 && b * s < 256) s = std::min<long>((256 + b - 1) / b, std::max(1, nkt / 8));  // one block per CU: at least fill the chip once
    s = std::min<long>(s, 128);
    s = std::min<long>(s, std::max<long>(1, 65535 / std::max<long>(zb, 1)));
    s = std::max<long>(1, s);
    // wave quantisation: the grid runs in waves of `slots` resident blocks (256 CUs x blocks per CU for this tile's LDS),
    // and a block's time is ~ K / splits -- 36 tiles x 15 splits on the one-block-per-CU 256x256 kernel is three waves
    // (256 + 256 + 28) where 36 x 7 is one.  Take the fewest splits within 5 % of the best waves/splits ratio.
    {
      const long slots = 256L * (tile == kTile256x256 ? 1 : tile == kTile128x128 ? 2 : tile == kTile128x64 ? 3 : 4);
      double best = 1e30;
      for (long c = 1; c <= s; ++c) best = std::min(best, (double)((b * c + slots - 1) / slots) / (double)c);
      for (long c = 1; c <= s; ++c)
        if ((double)((b * c + slots - 1) / slots) / (double)c <= best * 1.05) {
          s = c;
          break;
        }
    }
    plan.splits = (int)s;
  } else {
    if (p.splits <= 0) plan.splits = 1;
    const long sp = plan.splits;
    // measured with the lean epilogue (profiles/README.md, forced-tile sweep): the 128x128 tile wins from ~1 block per CU up
    // 256x256 (8 waves, one block per CU) from ~4 blocks per CU on deep contractions: 8192^3 1302 -> 1060 us, the head's
    // 3x3 bottleneck conv 2134 -> 1570 us; short-K or narrow problems lose to the 128x128 tile
    if (bf16 && p.N >= 256 && p.K >= 256 && (blocks(kTile256x256) * sp >= 1024 || (blocks(kTile256x256) * sp >= 200 && p.K >= 2048))) tile = kTile256x256;  // (4096^3: one block per CU, 1113 vs 883 TFLOP/s on 128x128)
    // output-bound GEMMs with a plain epilogue (MixFFN fc1 of stages 1 / 2: 131072 x 256 x 64, 32768 x 512 x 128; the head's pointwise
    // convolution over the teacher's 98304 rows): the ping-pong kernel's bf16 row image stores 16-byte pieces of whole rows
    // (29.6 against 38.4 us, 18.4 against 24.3 us; at 16384 x 512 the 64-wide tiles are still ahead)
    else if (bf16 && (p.N & 255) == 0 && p.K <= 1024 && blocks(kTile256x256) * sp >= 256 && !p.a_kstrided && !p.b_kstrided && p.A.conv != 1 &&
             p.B.conv != 1 && !p.res && !p.rowscale && p.beta == 0.f && !p.out_f32 && !p.atomic && p.c_patch_ow == 0)
      tile = kTile256x256;
    // N = 320 (64 x odd): the last 128-wide tile column would be half empty -- with enough blocks the 128x64 tile wins
    // (batch 64, M = 65536: q 42.2 -> 38.9 us, dfc1 110.8 -> 99.6 us; at batch 16 the 128x128 tile is still ahead)
    else if (p.N > 64 && (p.N & 127) > 0 && (p.N & 127) <= 64 && blocks(kTile128x64) * sp >= 2048) tile = kTile128x64;
    else if (p.N > 64 && blocks(kTile128x128) * sp >= 256) tile = kTile128x128;
    else if (blocks(kTile128x64) * sp >= 2048) tile = kTile128x64;
    else tile = kTile64x64;
    // Small grids (at most ~two waves of 128x128 tiles: the UDA step's encoder Linears, M = 2048...8192 rows): the kernel time is
    // (waves of resident blocks) x (time of one block), so pick the tile by that product.  Block time ~ c0 + c1 * k-tiles, fitted to
    // tools/gemm_sweep.py (profiles/r02_gemm_sweep.txt): 128x128 4 + 0.9 nkt us (2 blocks per CU), 128x64 3 + 0.75 nkt (3 per CU),
    // 64x64 2.5 + 0.6 nkt (4 per CU).  8192x1280x320: 128x128 26.1 -> 128x64 20.9 us; 8192x320x1280 stays on 64x64.
    if (tile != kTile256x256 && blocks(kTile128x128) * sp < 1024 && p.M > 64 && p.N > 64) {
      const double nk = (double)nkt;
      const double cost0 = (double)((blocks(kTile128x128) * sp + 511) / 512) * (4.0 + 0.9 * nk);
      // (round 4: the lean instance of the two small tiles -- gemm_lean.hip -- has a cheaper prologue / epilogue and a 0.3 us k-tile:
      // 16384 x 512 x 128 10.9 us on 64 x 64 tiles against 13.7 on 128 x 128, tools/dbg/pp_vs_lean.py)
      const bool lean = bf16 && !h.no_lean && cmda_gemm_lean_ok_(p);
      const double cost1 = (double)((blocks(kTile128x64) * sp + 767) / 768) * (lean ? 1.5 + 0.45 * nk : 3.0 + 0.75 * nk);
      const double cost2 = (double)((blocks(kTile64x64) * sp + 1023) / 1024) * (lean ? 1.2 + 0.3 * nk : 2.5 + 0.6 * nk);
      tile = cost0 <= cost1 && cost0 <= cost2 ? kTile128x128 : cost1 <= cost2 ? kTile128x64 : kTile64x64;
    }
  }
  if (h.tile >= 1 && h.tile <= 4) tile = (GemmTile)(h.tile - 1);  // caller's explicit tile choice (tuning sweeps, tests)
  plan.tile = tile;
  const bool small = tile == kTile128x64 || tile == kTile64x64;
  const bool ac = p.A.conv == 1, bc = p.B.conv == 1, aks = p.a_kstrided != 0, bks = p.b_kstrided != 0;  // conv == 2: patch view, plain fills
  // LDS-DMA path (bf16): every operand mode with aligned 16-byte chunks; operands too large for 32-bit tile arithmetic stay on the
  // register-staged kernel (zero-inserted inputs: the K-contiguous im2col operand A only)
  const bool kind_ok = (!ac && !bc) || (ac && !bc && !aks && !bks) || (!ac && bc && aks && bks);
  const bool glds = bf16 && !h.reg && kind_ok && gemm_dma_view_ok(p.A, ac && !p.A.reflect && !aks) && gemm_dma_view_ok(p.B, false);
  GemmParams q = p;   // the eligibility tests of the split-bf16 kernels see the resolved split count
  q.splits = plan.splits;
  // the fused bias gradient lives in the LDS-DMA kernels only (bf16: K-strided A; split-bf16: the lean weight-gradient form)
  const bool x3_lean = p.dtype == CMDA_F32X3 && !h.no_lean && cmda_gemm_x3_lean_ok_(q);
  if (p.colsum && !(glds ? aks : x3_lean)) return plan;
  plan.err = CMDA_OK;
  if (!glds) {
    // split-bf16: the encoders' Linear layers / data gradients (small grids: the 64 x 64 and 128 x 64 tile choices) on the LDS-DMA
    // instance, and every weight gradient it takes (split-K over the tokens chosen by the kernel's launcher, bias gradient fused)
    plan.family = p.dtype != CMDA_F32X3 ? kGemmReg : (small || aks || h.x3_lean) && !p.colstats && x3_lean ? kGemmX3Lean : kGemmX3Reg;
    if (plan.family == kGemmX3Lean) plan.tile = kTile64x64, plan.waves = 8;
    else if (tile == kTile256x256) plan.tile = kTile128x128;   // the 256x256 tile exists on the LDS-DMA path only
    return plan;
  }
  plan.waves = tile == kTile256x256 ? 8 : 4;
  // the 256x256 tile has three kernels: the ping-pong kernel (gemm_pp.hip: 32x32x16 MFMA, two wave groups alternating LDS reads and
  // MFMAs, bf16 epilogue image) for plain epilogues, gemm_wg.hip for the weight-gradient form, gemm_glds_kernel for the rest
  // Measured (profiles/r03_gemm_big.txt): the ping-pong kernel wins where the epilogue / short contraction dominates (K <= 1024:
  // 65536x1280x320 96 against 113 us, the head's pointwise data gradient 262144x1024x256 300 against 392 us) and on K-strided B
  // (8192^3 NN 863 against 778-837 TFLOP/s); long K-contiguous contractions and im2col views stay on gemm_glds_kernel (8192^3 NT
  // 1086 against 1024, the 3x3 bottleneck 1405 against 1776 us: the per-lane im2col address arithmetic sits in the LOAD segments)
  const bool pp_shape = h.ping_pong || (!ac && (p.K <= 1024 || bks));
  if (tile == kTile256x256 && !h.glds256 && pp_shape && !aks && !bc && !p.atomic && plan.splits == 1 && !p.res && !p.rowscale && p.beta == 0.f &&
      !p.out_f32 && p.c_patch_ow == 0 && !p.colsum)
    plan.family = kGemmPingPong;
  else if (tile == kTile256x256 && !h.glds256 && aks && bks && !ac && p.atomic && p.out_f32) plan.family = kGemmWgrad;
  // the encoders' Linear layers / data gradients on the two small tiles: the lean instance (fused column statistics: the general epilogue)
  else if (small && !p.colstats && !h.no_lean && cmda_gemm_lean_ok_(p)) plan.family = kGemmLean;
  else plan.family = kGemmGlds;
  if (plan.family == kGemmLean || plan.family == kGemmGlds) {
    plan.stages = plan_stages(h, tile, blocks(tile) * plan.splits, nkt / plan.splits);
    // The lean kernel's 2-stage configurations run on EIGHT waves (16 x 32 / 32 x 32 of the tile per wave): a lone workgroup's k-tile is
    // bound by how fast its waves can issue LDS-DMA pieces (0.3 us per 16 KiB with four waves), and twice the waves issue half the pieces
    // each -- 2048 x 320 x 320 5.05 -> 4.31 us, 8192 x 1280 x 320 18.6 -> 16.6, the step 60.2 -> 59.0 ms (the 4-stage configurations
    // measured the same on 4 and 8 waves and stay on 4)
    if (plan.family == kGemmLean && plan.stages == 2) plan.waves = 8;
  }
  return plan;
}

int run_plan(const GemmParams& p, const GemmPlan& plan, void* stream) {
  typedef int (*Launcher)(const GemmParams&, const GemmPlan&, void*);
  const Launcher glds[4] = {cmda_gemm_glds_t0_, cmda_gemm_glds_t1_, cmda_gemm_glds_t2_, cmda_gemm_glds_t3_};   // by GemmTile
  const Launcher run[8] = {nullptr, cmda_gemm_pp_, cmda_gemm_wg_, glds[plan.tile], cmda_gemm_lean_, cmda_gemm_reg_, cmda_gemm_x3_, cmda_gemm_x3_lean_};   // by GemmFamily
  return run[plan.family] ? run[plan.family](p, plan, stream) : plan.err;
}

// validate, then plan: `p` = the caller's block with batch2 normalised and the plan's split count
GemmPlan checked_plan(const cmda_gemm_params_t* pp, GemmParams& p) {
  GemmPlan none{CMDA_ERR_SHAPE, kGemmNone, kTile64x64, 0, 0, 0, false};
  if (!pp) return none;
  p = *pp;
  if (p.batch2 <= 0) p.batch2 = 1;
  auto fail = [&](int rc) { none.err = rc; return none; };
  if (p.M <= 0 || p.N <= 0 || p.batch <= 0) return fail(CMDA_OK);
  if (p.K <= 0) return fail(CMDA_ERR_SHAPE);
  if (p.atomic && !p.out_f32) return fail(CMDA_ERR_UNSUPPORTED);
  if (p.splits > 1 && !p.atomic) return fail(CMDA_ERR_UNSUPPORTED);
  if (p.atomic && (p.bias || p.act || p.res || p.rowscale)) return fail(CMDA_ERR_UNSUPPORTED);
  if (p.colstats && (p.atomic || p.splits > 1 || p.act || p.rowscale || p.c_patch_ow > 0 || p.a_kstrided || p.batch != 1 || p.batch2 != 1 || (p.N & 3) ||
                     p.colstats_rows <= 0 || (p.colstats_rows & 255) || p.colsum))
    return fail(CMDA_ERR_UNSUPPORTED);
  if (p.c_patch_ow > 0 && (p.atomic || p.res || p.batch != 1 || p.batch2 != 1 || p.c_patch_kh <= 0 || p.c_patch_kwci <= 0 ||
                           p.N != p.c_patch_kh * p.c_patch_kwci || p.M % p.c_patch_ow != 0 || (p.c_patch_kwci & 3)))
    return fail(CMDA_ERR_UNSUPPORTED);
  if (p.dtype != CMDA_F32 && p.dtype != CMDA_F32X3 && p.dtype != CMDA_BF16) return fail(CMDA_ERR_DTYPE);
  const GemmPlan plan = plan_gemm(p);
  p.splits = plan.splits;
  return plan;
}

}  // namespace

extern "C" int cmda_gemm(const cmda_gemm_params_t* pp, void* stream) {
  GemmParams p;
  const GemmPlan plan = checked_plan(pp, p);
  return run_plan(p, plan, stream);
}

// the plan as integers, no launch: out[0..6] = return code, family, tile, stages, waves, splits, general address path (tests/test_gemm_plan.py)
extern "C" int cmda_debug_gemm_plan(const cmda_gemm_params_t* pp, int32_t* out) {
  GemmParams p;
  const GemmPlan plan = checked_plan(pp, p);
  const int v[7] = {plan.err, plan.family, plan.tile, plan.stages, plan.waves, plan.splits, plan.general_addr};
  for (int i = 0; i < 7; ++i) out[i] = v[i];
  return CMDA_OK;
}

#ifdef CMDA_GEMM_TIMING
// the tuning build is ONE translation unit, so that every kernel stamps the same g_stamps array
#include "gemm_t0.hip"
#include "gemm_t1.hip"
#include "gemm_t2.hip"
#include "gemm_t3.hip"
#include "gemm_reg.hip"
#include "gemm_reg_f32_t0.hip"
#include "gemm_reg_f32_t1.hip"
#include "gemm_reg_f32_t2.hip"
#include "gemm_reg_bf16_t0.hip"
#include "gemm_reg_bf16_t1.hip"
#include "gemm_reg_bf16_t2.hip"
extern "C" int cmda_debug_gemm_stamps(unsigned long long* host_out) {
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 256 * 8) == hipSuccess ? 0 : -3;
}
#endif
