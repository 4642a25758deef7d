/* cmda_hip_ext6.h -- sixth extension of the C ABI of libcmda_hip.so: the per-stream training targets of the split train type
 * ('cs2dz_image+raw-isr_split': two streams, each self-trained on the teacher's pseudo-labels for that stream) in one kernel pair.
 *
 * include/cmda_hip.h (version 8) and the tables `cmdax_` .. `cmdax5_` (version 1 each) are frozen; entry points added after them
 * live here under the prefix `cmdax6_`, in the SAME shared library and with the same conventions:
 *  - returns 0 (CMDA_OK) or a negative CMDA_ERR_* code; never throws; a refused call launches nothing and writes nothing; every
 *    refusal is decided on the host before the launch;
 *  - every pointer is a device pointer; tensors are contiguous; `void* stream` (a hipStream_t) is the last argument;
 *  - stateless: no allocation, no host synchronisation; integer atomics only: results are identical from run to run, bit for bit.
 * cmdax6_abi_version() versions this table on its own; the versions of the earlier tables are not affected by it.
 */
#ifndef CMDA_HIP_EXT6_H
#define CMDA_HIP_EXT6_H
#include "cmda_hip_ext5.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CMDAX6_MAX_CLASSES 32   /* classes of a logit map (the per-pixel scores live in registers, as in cmda_pseudo_label) */

int cmdax6_abi_version(void);

/* Launch A.  logits0 / logits1: fp32 NHWC [B][h][w][nc] (the teacher's two outputs at low resolution); src_label int64 [B][H][W];
 * classes int64 [B][K], the classes drawn for ClassMix per sample, padded with -1.  Per full-resolution pixel and per map s:
 *   the bilinear up-sample of the map's nc scores (align_corners = False), cmda_pseudo_label's expression: the same bits;
 *   pseudo[s][b][Y][X] = the first arg-max;  prob = 1 / sum_c exp(score_c - max);  count[s] += (prob >= thr);
 *   mixed[s][b][Y][X]  = src_label[b][Y][X] where that label is one of classes[b][*], else pseudo[s][b][Y][X]
 * (the membership is evaluated once per pixel and serves both maps).  pseudo, mixed: int64 [2][B][H][W]; count: int32 [2],
 * ACCUMULATED (the caller zeroes it): one integer atomic per workgroup and map.  A map's half equals what cmda_pseudo_label followed by
 * cmda_class_mix_label gives for that map, bit for bit.
 * CMDA_ERR_SHAPE: nc < 1 or nc > CMDAX6_MAX_CLASSES; K < 1; B, h, w, H or W < 1; B*H*W > 2^31 - 1;
 * CMDA_ERR_UNSUPPORTED: a null pointer. */
int cmdax6_split_targets(const float* logits0, const float* logits1, const int64_t* src_label, const int64_t* classes, int64_t* pseudo,
                         int64_t* mixed, int* count, int B, int h, int w, int H, int W, int nc, int K, float thr, void* stream);

/* Launch B.  count int32 [2] as launch A left it; weight fp32 [2][B][H][W]:
 *   weight[s][b][Y][X] = 1 where src_label[b][Y][X] is one of classes[b][*]; elsewhere 0 in the first `top` and the last `bottom` rows
 *   and (float)((double)count[s] / (double)(B*H*W)) in the rows between -- cmda_pseudo_weight's expression, ClassMix'd against ones.
 * top + bottom beyond H is legal and zeroes every pixel outside the drawn classes.
 * CMDA_ERR_SHAPE: K < 1; B, H or W < 1; top or bottom < 0; B*H*W > 2^31 - 1;  CMDA_ERR_UNSUPPORTED: a null pointer. */
int cmdax6_split_weights(const int* count, const int64_t* src_label, const int64_t* classes, float* weight, int B, int H, int W, int K,
                         int top, int bottom, void* stream);

#ifdef __cplusplus
}
#endif
#endif
