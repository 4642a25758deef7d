/* cmda_hip_ext2.h -- second extension of the C ABI of libcmda_hip.so: sliding-window and multi-view (multi-scale / flip) evaluation.
 *
 * include/cmda_hip.h (version 8) and include/cmda_hip_ext.h (`cmdax_`, version 1) are frozen; entry points added after them live
 * here under the prefix `cmdax2_`, in the SAME shared library and with the same conventions:
 *  - returns 0 (CMDA_OK) or a negative CMDA_ERR_* code; never throws; a refused call launches nothing and writes nothing;
 *  - every pointer is a device pointer; tensors are contiguous; `void* stream` (a hipStream_t) is the last argument;
 *  - stateless: no allocation, no host synchronisation.
 * cmdax2_abi_version() versions this table on its own; cmda_abi_version() and cmdax_abi_version() are not affected by it.
 */
#ifndef CMDA_HIP_EXT2_H
#define CMDA_HIP_EXT2_H
#include "cmda_hip_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cmdax2_seg_scores `mode` */
#define CMDAX2_LABELS 0
#define CMDAX2_PROBS 1

int cmdax2_abi_version(void);

/* Evaluation tail of a segmentor under test_cfg.mode 'slide' (the reference's slide_inference + inference,
 * mmseg/models/segmentors/encoder_decoder.py:175-272) from the low-resolution logits of ALL windows of an image, in one launch.
 *
 * Window grid of the H x W network input (derived here from the scalars, as the reference derives it):
 *   gy = max(H - crop_h + stride_h - 1, 0) / stride_h + 1 rows of windows, gx likewise; K = gy * gx; window k = i * gx + j covers
 *   rows [y1, y2) with y2 = min(i * stride_h + crop_h, H), y1 = max(y2 - crop_h, 0), columns likewise: every window has the size
 *   ch x cw = min(crop_h, H) x min(crop_w, W).
 * logits: fp32 NHWC [K][B][hl][wl][nc], 1 <= nc <= CMDAX_MAX_CLASSES: the network's output for window k of image b.
 *   S1(y, x) = (sum over the windows k that cover (y, x), in the order of k, of U_k(y - y1_k, x - x1_k)) / (their number), with
 *              U_k = bilinear(logits_k -> ch x cw); a plain fp32 sum that starts from 0 and a real fp32 division;
 *   S2       = bilinear(S1 -> OH x OW) when (OH, OW) != (H, W), else S1, every S1 value rounded to fp32
 *   (align_corners = False; the arithmetic of cmda_upsample_logits_nchw per window, a sum, a division and a second
 *   cmda_upsample_logits_nchw, bit for bit).  `flip` (CMDAX_FLIP_*) is the flip the test pipeline applied to the network input:
 *   the value of S2 at (y, x) belongs to the output position (y, OW-1-x) for a horizontal flip, (OH-1-y, x) for a vertical one.
 * mode CMDAX2_LABELS: label_out uint8 [B][OH][OW] = first arg-max over the classes of S2 at the flipped-back position (the
 *   reference's soft-max is monotone: skipped).  Fused score (both or neither): gt [B][OH][OW] of dtype tag gt_dtype and conf
 *   int64 [(nc+1)*nc], ACCUMULATED -- exactly the counters of cmdax_seg_predict.  acc / accumulate are ignored.
 *   One window that covers the image (crop >= image) gives the labels and counters of cmdax_seg_predict.
 * mode CMDAX2_PROBS: acc fp32 NCHW [B][nc][OH][OW]; acc[b][c] = (accumulate ? acc[b][c] : 0) + softmax_c(S2) at the flipped-back
 *   position (the reference's `inference` output, summed over the views by its aug_test).  label_out is ignored; gt and conf
 *   must be null.
 * CMDA_ERR_SHAPE: nc outside [1, 32], B < 0, a size / crop / stride / hl / wl < 1, K*B >= 2^31, B*OH*OW >= 2^31;
 * CMDA_ERR_DTYPE: bad gt_dtype; CMDA_ERR_UNSUPPORTED: bad mode or flip, gt without conf or conf without gt, gt / conf in
 * mode CMDAX2_PROBS, a null output of the mode. */
int cmdax2_seg_scores(const float* logits, int mode, uint8_t* label_out, float* acc, int accumulate, const void* gt, int gt_dtype,
                      int64_t* conf, int B, int hl, int wl, int H, int W, int crop_h, int crop_w, int stride_h, int stride_w, int OH,
                      int OW, int nc, int flip, int ignore_index, void* stream);

/* Labels of the averaged probabilities of n views (the end of the reference's aug_test, encoder_decoder.py:287-304):
 * label_out uint8 [B][OH][OW] = first arg-max over c of acc[b][c][y][x] / (float)n, acc fp32 NCHW [B][nc][OH][OW] as
 * cmdax2_seg_scores accumulates it.  Fused score (both or neither): gt / conf as above.
 * CMDA_ERR_SHAPE: nc outside [1, 32], B < 0, a size < 1, n < 1, B*OH*OW >= 2^31; CMDA_ERR_DTYPE: bad gt_dtype;
 * CMDA_ERR_UNSUPPORTED: gt without conf or conf without gt. */
int cmdax2_prob_predict(const float* acc, uint8_t* label_out, const void* gt, int gt_dtype, int64_t* conf, int B, int OH, int OW,
                        int nc, int n, int ignore_index, void* stream);

#ifdef __cplusplus
}
#endif
#endif
