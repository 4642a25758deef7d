// gemm_reg.hip -- dispatch of the register-staged GEMM kernel: the exact-fp32 parity mode and the bf16 operand views the
// LDS-DMA path does not take (transposed-conv zero insertion, reflection padding, unaligned chunks).  The instantiations
// live in gemm_reg_{f32,bf16}_t{0,1,2}.hip, one (dtype, tile) per translation unit.  Templates: gemm_kernels.h.
#include "gemm_kernels.h"

int cmda_gemm_reg_(const cmda_gemm_params_t& p, const GemmPlan& plan, void* stream) {
  const GemmTile t = plan.tile;
  if (p.dtype == CMDA_F32) return t == kTile128x128 ? cmda_gemm_reg_f32_t0_(p, stream) : t == kTile128x64 ? cmda_gemm_reg_f32_t1_(p, stream) : cmda_gemm_reg_f32_t2_(p, stream);
  return t == kTile128x128 ? cmda_gemm_reg_bf16_t0_(p, stream) : t == kTile128x64 ? cmda_gemm_reg_bf16_t1_(p, stream) : cmda_gemm_reg_bf16_t2_(p, stream);
}
