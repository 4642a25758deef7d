/* cmda_hip_ext3.h -- third extension of the C ABI of libcmda_hip.so: the ISR augmentations (sky mask, sensor noise) of the training step.
 *
 * include/cmda_hip.h (version 8), include/cmda_hip_ext.h (`cmdax_`, version 1) and include/cmda_hip_ext2.h (`cmdax2_`, version 1) are
 * frozen; entry points added after them live here under the prefix `cmdax3_`, in the SAME shared library and with the same conventions:
 *  - returns 0 (CMDA_OK) or a negative CMDA_ERR_* code; never throws; a refused call launches nothing and writes nothing;
 *  - every pointer is a device pointer unless it says HOST; tensors are contiguous; `void* stream` (a hipStream_t) is the last argument;
 *  - stateless: no allocation, no host synchronisation; no float atomics (integer ones only): results are run-to-run identical;
 *  - per-sample parameters are read from DEVICE memory by the kernels, so a captured launch sequence sees new draws at every replay.
 * cmdax3_abi_version() versions this table on its own; the versions of the earlier tables are not affected by it.
 */
#ifndef CMDA_HIP_EXT3_H
#define CMDA_HIP_EXT3_H
#include "cmda_hip_ext2.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CMDAX3_SKY_CLASS 10      /* Cityscapes train id of 'sky' */
#define CMDAX3_SKY_MIN_PIXELS 10 /* fewer sky pixels: the sample passes through */
#define CMDAX3_SKY_MAX_W 8192    /* one image row's prefix sum lives in LDS */

int cmdax3_abi_version(void);

/* Bytes of the workspace `ws` of cmdax3_sky_mask: per sample 4 int32 statistics, H int32 row counts, H*W uint16 window counts and
 * H*W uint8 row-window counts.  The contents need no initialisation and mean nothing between calls. */
int64_t cmdax3_sky_mask_ws_bytes(int B, int H, int W);

/* sky_mask_transform of the reference (mmseg/models/utils/dacs_transforms.py:134-171) for a batch, in three launches.
 * label [B][H][W] of dtype tag label_dtype (CMDAX_U8 / CMDAX_I64); isr, out fp32 NCHW [B][C][H][W], C in {1, 3} (out == isr is
 * allowed); bank uint8 [n_bank][bank_h][bank_w], bank_h x bank_w must be H x W.
 * prm int32 [B][4] per sample: {k, bank index, the bits of fp32 lambda_erase_expansion, the bits of fp32 noise_intensity};
 * src_row int32 [B][H], src_col int32 [B][W]: the bank row / column that lands on every output row / column (the chunk shuffle of
 * :162-166 expanded, any permutation; entries are clamped into the image, the bank index into [0, n_bank));
 * enable int32 [B] or null (all on).  Per sample, with sky = (label == 10):
 *   fewer than 10 sky pixels, enable == 0, or k not odd in [21, 61]  ->  out = isr, bit for bit;
 *   S = number of sky pixels in the k x k window clipped to the image (integer);  expansion = (S > 0);
 *   weight = sky ? 0 : (float)S / (float)(k*k)  (one correctly rounded division: avg_pool2d with zero padding counted in the divisor);
 *   max, min of weight over the sample from the integer max / min of (sky ? 0 : S): exact and independent of the block order;
 *   wn = (weight - min) / (max - min), and wn = 0 where max == min (an all-sky sample; the reference divides 0 by 0 there);
 *   blur_w = 1 - clamp(wn + lambda * (wn != 0), 0, 1);
 *   out = clamp(isr * (1 - sky) * blur_w + (bank/128 - 1)[src_row[y]][src_col[x]] * expansion * intensity, -1, 1) on every channel.
 * dbg_expansion / dbg_blur_w: fp32 [B][H][W] or null; receive expansion and blur_w (0 and 1 for a sample that passes through).
 * k_check: HOST int[B] or null: the k values as the host knows them, checked here (the device copy cannot be read without a sync).
 * CMDA_ERR_SHAPE: C outside {1, 3}, B < 0, a size < 1, W > CMDAX3_SKY_MAX_W, B*C*H*W >= 2^31, n_bank < 1, a bank that is not H x W,
 * a k_check entry that is even or outside [21, 61]; CMDA_ERR_DTYPE: bad label_dtype; CMDA_ERR_UNSUPPORTED: a null pointer other than
 * enable, dbg_* and k_check. */
int cmdax3_sky_mask(const void* label, int label_dtype, const float* isr, const uint8_t* bank, const int32_t* prm, const int32_t* src_row,
                    const int32_t* src_col, const int32_t* enable, float* out, float* dbg_expansion, float* dbg_blur_w, void* ws,
                    const int* k_check, int B, int C, int H, int W, int n_bank, int bank_h, int bank_w, void* stream);

/* Standard-normal fields from a counter-based generator: Philox4x32-10 keyed by the 64-bit seed, counter = (pixel / 4, sample, call
 * offset, field), and Box-Muller on the four words (pixel % 4 picks one of the four normals).  out fp32 [3][B][H][W]: field f of
 * sample b.  The call offset is `offset` + *offset_dev (offset_dev: DEVICE int64 or null), in [0, 2^62).
 * CMDA_ERR_SHAPE: B < 0, a size < 1, B*H*W >= 2^31; CMDA_ERR_UNSUPPORTED: null out. */
int cmdax3_randn_fields(float* out, int B, int H, int W, uint64_t seed, int64_t offset, const int64_t* offset_dev, void* stream);

/* add_noise_on_isr of the reference (dacs_transforms.py:186-211) on channel 0 of isr, the result copied to all C channels of out
 * (mmseg/models/uda/dacs.py:754-755).  isr, out fp32 NCHW [B][C][H][W], C in {1, 3}, out != isr.
 * prm int32 [B][4] per sample: {blur gate, bits of fp32 t1, bits of fp32 t2, bits of fp32 intensity}; enable int32 [B] or null:
 * enable == 0 copies the sample's C channels through.  With x = isr[b][0]:
 *   blur (host flag) and the sample's blur gate: x = bilinear(avg_pool2d(x, 2) -> H x W), align_corners = False, the pooled size is
 *     floor(H/2) x floor(W/2) (the arithmetic of F.avg_pool2d + F.interpolate in fp32);
 *   noise (host flag): x = x * (|n1| < t1);  x = x + n3 * intensity * (|n2| < t2);  x = clamp(x, -1, 1).
 * Fields: n1, n2, n3 fp32 [B][H][W] each (all three or none).  With none given they are generated in the kernel by the device
 * function behind cmdax3_randn_fields from (seed, offset + *offset_dev): bit-equal to feeding that entry point's output.
 * CMDA_ERR_SHAPE: C outside {1, 3}, B < 0, a size < 1 (< 2 with blur), B*C*H*W >= 2^31; CMDA_ERR_UNSUPPORTED: null isr / out / prm,
 * out == isr, some but not all of n1, n2, n3. */
int cmdax3_isr_noise(const float* isr, float* out, const float* n1, const float* n2, const float* n3, const int32_t* prm,
                     const int32_t* enable, int B, int C, int H, int W, int blur, int noise, uint64_t seed, int64_t offset,
                     const int64_t* offset_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
