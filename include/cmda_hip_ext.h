/* cmda_hip_ext.h -- extension of the C ABI of libcmda_hip.so (include/cmda_hip.h, frozen at version 8).
 *
 * Entry points added after the core table was frozen live here under the prefix `cmdax_`, in the SAME shared library and with the
 * same conventions as the core header:
 *  - returns 0 (CMDA_OK) or a negative CMDA_ERR_* code; never throws; a refused call launches nothing and writes nothing;
 *  - every pointer is a device pointer; tensors are contiguous; `void* stream` (a hipStream_t) is the last argument;
 *  - stateless: no allocation, no host synchronisation.
 * cmdax_abi_version() versions this table on its own; cmda_abi_version() is not affected by it.
 */
#ifndef CMDA_HIP_EXT_H
#define CMDA_HIP_EXT_H
#include "cmda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* integer label tensors: dtype tags of the `gt` / `pred` arguments below */
#define CMDAX_U8 0
#define CMDAX_I64 1
/* cmdax_seg_predict `flip`: the flip the test pipeline applied to the network input, undone on the label map */
#define CMDAX_FLIP_NONE 0
#define CMDAX_FLIP_HORIZONTAL 1
#define CMDAX_FLIP_VERTICAL 2
#define CMDAX_MAX_CLASSES 32

int cmdax_abi_version(void);

/* Evaluation tail of a segmentor in one launch (the reference's whole_inference + inference + simple_test,
 * mmseg/models/segmentors/encoder_decoder.py:897-984, test_cfg.mode 'whole'):
 *   S1 = bilinear(logits -> H x W), S2 = bilinear(S1 -> OH x OW) when (OH, OW) != (H, W), else S1 (align_corners = False, the
 *   arithmetic of cmda_upsample_logits_nchw applied once or twice); label_out[b][y][x] = first arg-max over the classes of S2 at
 *   (y, OW-1-x) for a horizontal flip, (OH-1-y, x) for a vertical one, (y, x) for none.  The reference's soft-max is monotone: skipped.
 * logits: fp32 NHWC [B][h][w][nc], 1 <= nc <= CMDAX_MAX_CLASSES; label_out: uint8 [B][OH][OW]; B*OH*OW < 2^31.
 * Fused score (both or neither): gt [B][OH][OW] of dtype tag gt_dtype, in the frame of label_out; conf int64 [(nc+1)*nc],
 *   ACCUMULATED (the caller clears it): for every pixel with gt != ignore_index, conf[g*nc + label] += 1 with g = gt when
 *   0 <= gt < nc, else nc (the row of labels that are out of range but not ignored: the reference counts their predictions in the
 *   predicted area and drops them from the label area, mmseg/core/evaluation/metrics.py:75-86).  Integer counters: exact and
 *   independent of the order of the blocks.
 * CMDA_ERR_SHAPE: nc outside [1, 32], a size < 1, B*OH*OW >= 2^31; CMDA_ERR_DTYPE: bad gt_dtype;
 * CMDA_ERR_UNSUPPORTED: bad flip, gt without conf or conf without gt. */
int cmdax_seg_predict(const float* logits, uint8_t* label_out, const void* gt, int gt_dtype, int64_t* conf, int B, int h, int w,
                      int H, int W, int OH, int OW, int nc, int flip, int ignore_index, void* stream);

/* The same counters from label maps that already exist: pred and gt hold n labels each (dtype tags pred_dtype, gt_dtype);
 * conf int64 [(nc+1)*nc], ACCUMULATED, rows as above.  A prediction outside [0, nc) is dropped from every count.
 * CMDA_ERR_SHAPE: nc outside [1, 32], n < 0; CMDA_ERR_DTYPE: bad dtype tag. */
int cmdax_confusion_update(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int64_t* conf, int64_t n, int nc,
                           int ignore_index, void* stream);

#ifdef __cplusplus
}
#endif
#endif
