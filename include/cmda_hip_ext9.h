/* cmda_hip_ext9.h -- ninth extension of the C ABI of libcmda_hip.so: the feature-consistency loss of the `isr_no_fusion` route of
 * DACS (mmseg/models/segmentors/encoder_decoder.py:833-848: lambda * F.mse_loss(f_image[i], f_events[i].detach()) summed over the
 * four feature levels) -- the loss and its gradient with respect to the image features, for up to four levels in ONE launch.
 *
 * include/cmda_hip.h (version 8) and the tables `cmdax_` .. `cmdax8_` (version 1 each) are frozen; entry points added after them
 * live here under the prefix `cmdax9_`, in the SAME shared library and with the same conventions:
 *  - returns 0 (CMDA_OK) or a negative CMDA_ERR_* code; never throws; a refused call launches nothing and writes nothing; every
 *    refusal is decided on the host before the launch;
 *  - every pointer inside a descriptor is a device pointer; the descriptor array itself is HOST memory, read during the call;
 *    `void* stream` (a hipStream_t) is the last argument;
 *  - stateless: no allocation, no host synchronisation.
 * cmdax9_abi_version() versions this table on its own; the versions of the earlier tables are not affected by it.
 */
#ifndef CMDA_HIP_EXT9_H
#define CMDA_HIP_EXT9_H
#include "cmda_hip_ext8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CMDAX9_MAX_LEVELS 4

/* One feature level.  a: the image features, b: the features they are pulled towards (read only, no gradient), both [R, C] in the
 * feature dtype with row strides lda / ldb (elements): either may be a block of a wider buffer.  grad: NULL, or the block [R, C]
 * (row stride ldg, elements, ignored when grad is NULL) the gradient with respect to `a` is ADDED into, in the gradient dtype. */
typedef struct {
  const void* a;
  const void* b;
  void* grad;
  int64_t R;
  int64_t lda;
  int64_t ldb;
  int64_t ldg;
  int32_t C;
  int32_t reserved;   /* 0 */
} cmdax9_level_t;

int cmdax9_abi_version(void);

/* Floats of the partial-sum workspace of cmdax9_feat_consis (one per workgroup, at most 256 + n_levels); reads only R and C of each
 * descriptor.  -1 where
 * cmdax9_feat_consis would return CMDA_ERR_SHAPE for n_levels, an R or a C, or levels is NULL.  feat_dtype: CMDA_F32 or CMDA_BF16
 * (the workgroups are cut by 16-byte pieces of the features); -1 for another tag. */
int64_t cmdax9_ws_floats(const cmdax9_level_t* levels, int n_levels, int feat_dtype);

/* With n_l = R_l * C_l, d = a - b taken in fp32 and g = gscale[0] (gscale: fp32 [1] on the device, NULL = 1):
 *   level_loss[l] = lambda * sum(d^2) / n_l        (fp32 [n_levels], may be NULL)
 *   loss[0]       = sum_l level_loss[l]            (fp32 [1], added in level order)
 *   grad_l       += g * lambda * (2 / n_l) * d     (every level whose grad is not NULL)
 * One kernel, three modes decided by the pointers: loss only (every grad NULL), gradient only (loss NULL: level_loss, ticket and
 * partials_ws are not touched and may be NULL), both.  Deterministic: no float atomics; every workgroup leaves one partial sum in
 * partials_ws (cmdax9_ws_floats(...) floats, contents on entry do not matter), the last workgroup to arrive -- an integer ticket in
 * the caller-owned int32 `ticket`, zero before the launch and zero again after it -- folds them in index order; two launches on the
 * same inputs give bit-identical results.  16-byte accesses where the base pointers and the row strides of a level keep every
 * 16-byte piece of a row aligned, element accesses for the rest of a row (C no multiple of the piece) or for the whole level.
 * feat_dtype: CMDA_F32 or CMDA_BF16; grad_dtype: the same, or CMDA_F32 under CMDA_BF16 features.
 * CMDA_ERR_SHAPE: n_levels outside 1..4, an R or a C below 1, lda / ldb below C, ldg below C where grad is not NULL, R * ceil(C / piece)
 * of a level at or above 2^31;
 * CMDA_ERR_DTYPE: another dtype tag, CMDA_BF16 gradients under CMDA_F32 features;
 * CMDA_ERR_UNSUPPORTED: levels NULL (with n_levels in range), a NULL a / b, loss NULL and every grad NULL, loss given without ticket or
 * partials_ws.  Shapes are checked first, then the dtypes, then the pointers. */
int cmdax9_feat_consis(const cmdax9_level_t* levels, int n_levels, float lambda, const float* gscale, float* loss, float* level_loss,
                       int* ticket, float* partials_ws, int feat_dtype, int grad_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif
