/* cmda_hip_ext8.h -- eighth extension of the C ABI of libcmda_hip.so: the tail of the ResNet BasicBlock pairs of the convolutional
 * fusion module (`fusion_module=dict(type='ConvertAvgFusion')`, mmseg/models/fusion/convert_avg_fusion.py, backbones/resnet.py:15-100)
 * -- BatchNorm 2, the residual add, ReLU and the average of the image-side and the event-side block, fused, for up to four feature
 * levels per launch -- its backward, and the statistics-only half of cmda_bn_train_fwd.
 *
 * include/cmda_hip.h (version 8) and the tables `cmdax_` .. `cmdax7_` (version 1 each) are frozen; entry points added after them
 * live here under the prefix `cmdax8_`, in the SAME shared library and with the same conventions:
 *  - returns 0 (CMDA_OK) or a negative CMDA_ERR_* code; never throws; a refused call launches nothing and writes nothing; every
 *    refusal is decided on the host before the launch;
 *  - every pointer inside a descriptor is a device pointer; the descriptor array itself is HOST memory, read during the call;
 *    tensors are contiguous; `void* stream` (a hipStream_t) is the last argument;
 *  - stateless: no allocation, no host synchronisation.
 * cmdax8_abi_version() versions this table on its own; the versions of the earlier tables are not affected by it.
 */
#ifndef CMDA_HIP_EXT8_H
#define CMDA_HIP_EXT8_H
#include "cmda_hip_ext7.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CMDAX8_MAX_LEVELS 4
#define CMDAX8_MAX_GROUPS 8

/* One BasicBlock of a level.  z: the output of conv2, x: the input of the block (the identity path), both [groups*M, C] in the storage
 * dtype; mean / rstd: fp32 [groups][C], the statistics of z per row block (batch statistics in train mode, the running ones repeated in
 * eval mode); gamma / beta: fp32 [C].  The last four are read by cmdax8_resavg_bwd only (cmdax8_resavg_fwd ignores them): dz, dres
 * [groups*M, C] in the storage dtype (out), dgamma / dbeta fp32 [C] (accumulated into). */
typedef struct {
  const void* z;
  const void* x;
  const float* mean;
  const float* rstd;
  const float* gamma;
  const float* beta;
  void* dz;
  void* dres;
  float* dgamma;
  float* dbeta;
} cmdax8_branch_t;

/* One feature level: the image-side block br[0], the event-side block br[1].  out (forward, written) / dout (backward, read):
 * [groups*M, C] in the storage dtype, possibly a row slice of a larger buffer of the same row pitch C.  M: rows PER GROUP. */
typedef struct {
  cmdax8_branch_t br[2];
  void* out;
  const void* dout;
  int64_t M;
  int32_t C;
  int32_t reserved;   /* 0 */
} cmdax8_level_t;

int cmdax8_abi_version(void);

/* out = 0.5 * (relu(bn_i(z_i) + x_i) + relu(bn_e(z_e) + x_e)) for n_levels levels in ONE launch, bn(z) = (z - mean) * rstd * gamma + beta
 * with the statistics row g for the rows [g*M, (g+1)*M) of a level.  Nothing else is written.  4 reads and 1 write of every map.
 * dtype: CMDA_F32 or CMDA_BF16 (storage; the arithmetic is fp32).  16-byte accesses where C % 8 == 0 (bf16) and every map is
 * 16-byte aligned, 8-byte ones otherwise.
 * CMDA_ERR_UNSUPPORTED: levels NULL (with n_levels in range) or a NULL z / x / mean / rstd / gamma / beta / out;
 * CMDA_ERR_SHAPE: n_levels outside 1..4, groups outside 1..8, C < 4 or C % 4 != 0, M < 1, groups*M*C >= 2^31 for a level;
 * CMDA_ERR_DTYPE: another dtype tag.  Shapes are checked first, then the dtype, then the pointers. */
int cmdax8_resavg_fwd(const cmdax8_level_t* levels, int n_levels, int groups, int dtype, void* stream);

/* Floats of the workspace of cmdax8_resavg_bwd: per level, branch and group 33 x 2C (32 slots of partial sums and their fold, the
 * layout of cmda_bn_ws_floats).  Reads only C of each descriptor.  -1 where cmdax8_resavg_bwd would return CMDA_ERR_SHAPE for n_levels,
 * groups or a C, or levels is NULL. */
int64_t cmdax8_ws_floats(const cmdax8_level_t* levels, int n_levels, int groups);

/* The backward of cmdax8_resavg_fwd.  Per branch, with pre = bn(z) + x, g = 0.5 * dout * [pre > 0] and xhat = (z - mean) * rstd (the
 * masks are recomputed, nothing of the forward pass is stored):
 *   s1 = sum_rows g, s2 = sum_rows g * xhat                               (per group and channel)
 *   dz = gamma * rstd * (g - s1 / M - xhat * s2 / M),   dres = g,   dgamma += sum_groups s2,   dbeta += sum_groups s1
 * Two passes over the maps for all levels -- one launch that reduces (5 reads), one that applies (5 reads, 4 writes) -- with the
 * clearing of the workspace (a kernel) in front and the fold of the 32 slots, which also adds into dgamma / dbeta, in between.
 * ws: cmdax8_ws_floats(...) floats, 16-byte aligned; contents on entry do not matter.
 * Refusals as cmdax8_resavg_fwd, a NULL dout / dz / dres / dgamma / dbeta / ws included. */
int cmdax8_resavg_bwd(const cmdax8_level_t* levels, int n_levels, int groups, float* ws, int dtype, void* stream);

/* The statistics half of cmda_bn_train_fwd: the reduction over x [groups*M, C] (skipped when ws_has_stats: a GEMM epilogue left the
 * sums in ws, which is then handed back zeroed), then its finalize -- mean / rstd [groups][C] written, running_mean / running_var
 * (may both be NULL) updated group after group in `order` (HOST, NULL = 0, 1, 2, ..).  No map is written.  groups, order, ws_has_stats
 * and ws (cmda_bn_ws_floats(C) floats per group) mean what they mean there, and the same refusals apply. */
int cmdax8_bn_stats(const void* x, float* mean, float* rstd, float* running_mean, float* running_var, float* ws, int64_t M, int C,
                    float eps, float momentum, int groups, const int* order, int ws_has_stats, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif
