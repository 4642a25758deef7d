/* cmda_hip_ext7.h -- seventh extension of the C ABI of libcmda_hip.so: the OHEM pixel sampler of the decode heads
 * (`sampler=dict(type='OHEMPixelSampler', ...)`, mmseg/core/seg/sampler/ohem_pixel_sampler.py) and the exact order-statistic select
 * it is built on.
 *
 * include/cmda_hip.h (version 8) and the tables `cmdax_` .. `cmdax6_` (version 1 each) are frozen; entry points added after them
 * live here under the prefix `cmdax7_`, in the SAME shared library and with the same conventions:
 *  - returns 0 (CMDA_OK) or a negative CMDA_ERR_* code; never throws; a refused call launches nothing and writes nothing; every
 *    refusal is decided on the host before the launch;
 *  - every pointer is a device pointer; tensors are contiguous; `void* stream` (a hipStream_t) is the last argument;
 *  - stateless: no allocation, no host synchronisation; integer atomics only (no float atomic anywhere): results are identical from
 *    run to run, bit for bit.
 * cmdax7_abi_version() versions this table on its own; the versions of the earlier tables are not affected by it.
 */
#ifndef CMDA_HIP_EXT7_H
#define CMDA_HIP_EXT7_H
#include "cmda_hip_ext6.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CMDAX7_MAX_CLASSES 32   /* classes of a logit map (the per-pixel scores live in registers, as in cmda_ce_upsample_fwd) */
#define CMDAX7_MODE_THRESH 0    /* key = softmax probability of the label; hard = below max(k-th smallest, thresh) */
#define CMDAX7_MODE_LOSS 1      /* key = per-pixel cross-entropy; hard = at or above the (min_kept * B)-th largest */

int cmdax7_abi_version(void);

/* Bytes of the workspace `ws` of the two calls below: the counters of the radix select (a few KB) followed by room for n_keys fp32
 * keys.  cmdax7_select_kth reads the caller's array: n_keys = 0.  cmdax7_ohem_weight keeps its keys there: n_keys = B*H*W.
 * Returns -1 for n_keys < 0 or beyond 2^31 - 1.  `ws` must be 16-byte aligned; its contents on entry do not matter (every call clears
 * its counters with a kernel of its own), and nothing in it outlives the call. */
int64_t cmdax7_ws_bytes(int64_t n_keys);

/* out[0] = the k-th smallest (k counted from 0) of the n fp32 values keys[0..n), exactly: the bit pattern of an element of the array,
 * equal to sort(keys)[k].  k: device int32[1], read on the device (clamped to [0, n - 1]).  Order: the total order of the IEEE bit
 * patterns (-0.0 below +0.0, NaNs of positive sign above +inf); keys are not modified.
 * Most-significant-digit radix select over an order-preserving uint32 image of the keys, 11 / 11 / 10 bits: four launches (histogram;
 * two refinements, each of which redoes the prefix scan of the level before it in every workgroup; the final scan) plus the kernel that
 * clears the counters.  Histograms are integer counts in LDS, flushed with integer atomics.
 * CMDA_ERR_SHAPE: n < 1 or n > 2^31 - 1;  CMDA_ERR_UNSUPPORTED: a null pointer. */
int cmdax7_select_kth(const float* keys, int64_t n, const int* k, float* out, void* ws, void* stream);

/* The OHEM pixel sampler.  logits: fp32 NHWC [B][h][w][nc]; label int64 [B][H][W]; weight fp32 [B][H][W] (out).
 * Per full-resolution pixel the nc scores are the bilinear up-sample (align_corners = False) cmda_ce_upsample_fwd computes: the same
 * bits.  A pixel is valid when its label is not ignore_index and lies in [0, nc); n_valid counts the valid pixels; batch_kept =
 * min_kept * B.
 *   CMDAX7_MODE_THRESH: key = softmax(scores)[label]; kth = the key of index min(batch_kept, n_valid - 1) in ascending order;
 *     threshold = max(kth, thresh) (thresh alone when n_valid = 0); weight = 1 where valid and key < threshold, else 0.
 *   CMDAX7_MODE_LOSS (thresh is not read): key = logsumexp(scores) - scores[label]; threshold = the batch_kept-th largest key (the
 *     smallest key when batch_kept >= n_valid; +inf when n_valid = 0); weight = 1 where valid and key >= threshold, else 0.  Keys that
 *     tie with the threshold exactly are ALL selected (the reference's unstable sort keeps an unspecified subset of them).
 * Four launches (keys + n_valid + first histogram; two refinements; weights) plus the kernel that clears the counters.
 * threshold_out: fp32[1] or NULL.  After the call the first B*H*W floats behind the counters of `ws` (ws + cmdax7_ws_bytes(0)) hold the
 * keys, invalid pixels as the bit pattern 0xFFFFFFFF.
 * CMDA_ERR_SHAPE: nc < 1 or nc > CMDAX7_MAX_CLASSES; B, h, w, H or W < 1; B*H*W > 2^31 - 1; min_kept < 2;
 * CMDA_ERR_UNSUPPORTED: a null pointer (threshold_out excepted); a mode that is neither of the two. */
int cmdax7_ohem_weight(const float* logits, const int64_t* label, float* weight, float* threshold_out, void* ws, int B, int h, int w,
                       int H, int W, int nc, int ignore_index, int mode, float thresh, int min_kept, void* stream);

#ifdef __cplusplus
}
#endif
#endif
