/* cmda_hip_ext4.h -- fourth extension of the C ABI of libcmda_hip.so: the multi-parameter ISR (three-channel "shift_3_channel" ISR with
 * an output window) and the cow-mask dropout of the source ISR.
 *
 * include/cmda_hip.h (version 8) and the tables `cmdax_`, `cmdax2_`, `cmdax3_` (version 1 each) are frozen; entry points added after
 * them live here under the prefix `cmdax4_`, in the SAME shared library and with the same conventions:
 *  - returns 0 (CMDA_OK) or a negative CMDA_ERR_* code; never throws; a refused call launches nothing and writes nothing;
 *  - every pointer is a device pointer unless it says HOST; tensors are contiguous; `void* stream` (a hipStream_t) is the last argument;
 *  - stateless: no allocation, no host synchronisation; no float atomics (integer ones only): results are run-to-run identical;
 *  - per-sample parameters are read from DEVICE memory by the kernels, so a captured launch sequence sees new draws at every replay.
 *    A value the kernels read from device memory cannot be checked by the host without a sync: the kernels clamp it into the legal
 *    range (no out-of-bounds access whatever the table holds), and the caller may pass the values as the HOST knows them to be checked.
 * cmdax4_abi_version() versions this table on its own; the versions of the earlier tables are not affected by it.
 */
#ifndef CMDA_HIP_EXT4_H
#define CMDA_HIP_EXT4_H
#include "cmda_hip_ext3.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CMDAX4_ISR_MAX_C 3     /* channels (parameter rows) of one cmdax4_isr_multi call */
#define CMDAX4_ISR_ROW 12      /* int32 words per parameter row */
#define CMDAX4_COW_MAX_K 255   /* taps of the cow-mask blur: the reference's 195 (max_sigma 16) with room */
#define CMDAX4_COW_TILE 32     /* the column pass works on 32 x 32 tiles: one partial (sum, sum of squares) per tile */

int cmdax4_abi_version(void);

/* C ISR channels of one gray map (get_image_change_from_pil of mmseg/datasets/utils.py:108-152 once per parameter row, the loops of
 * cityscapes_ic.py:225-230, dark_zurich_ic.py and dacs.py:746-751), in three launches for the whole batch.
 * gray uint8 [B][H][W]; lut fp32 [256] (log of the value range: one range per call); out fp32 [B][C][OH][OW].
 * prm int32 [C][12], one row per channel: {bits of fp32 threshold, bits of fp32 clip range (both already multiplied by the log span,
 *   as cmda_isr_from_gray takes them), ndir, dy0, dx0, dy1, dx1, dy2, dx2, dy3, dx3, unused}.  ndir is 2 or 4 (any other value is
 *   read as 2).
 * win int32 [B][3] or null, one row per sample: {x0, y0, flip}.  Null: OH x OW must be H x W and the whole map is written.  Otherwise
 *   out[b][c][oy][ox] = full[b][c][y0 + oy][x0 + (flip ? OW - 1 - ox : ox)]; x0 / y0 are clamped into [0, W - OW] / [0, H - OH].
 * mm uint32 [B][C][4][4]: workspace (initialised here).
 * Channel c is, bit for bit, what cmda_isr_from_gray gives for row c's parameters on the whole H x W map: the min / max
 * normalisation is over the whole map whatever the window.
 * ndir_check: HOST int[C] or null; win_check: HOST int[B][3] or null: the values as the host knows them, checked here.
 * CMDA_ERR_SHAPE: C outside 1..3, B < 0, a size < 1, OH > H, OW > W, (no window and OH x OW != H x W), B*C*OH*OW or B*H*W >= 2^31,
 * an ndir_check entry outside {2, 4}, a win_check row whose window leaves the map or whose flip is not 0 / 1;
 * CMDA_ERR_UNSUPPORTED: a null pointer other than win, ndir_check, win_check. */
int cmdax4_isr_multi(const uint8_t* gray, const float* lut, const int32_t* prm, const int32_t* win, uint32_t* mm, float* out,
                     const int* ndir_check, const int* win_check, int B, int C, int H, int W, int OH, int OW, void* stream);

/* Bytes of the workspace of cmdax4_cow_mask: per sample ceil(H/32)*ceil(W/32) pairs of doubles (tile sum, tile sum of squares), then
 * two fp32 planes (row pass, smooth field).  0 for an illegal (B, H, W, K).  Contents need no initialisation. */
int64_t cmdax4_cow_mask_ws_bytes(int B, int H, int W, int K);

/* cow_masks of the reference (mmseg/datasets/utils.py:171-200) for a batch and its use at cityscapes_ic.py:263-266, three launches:
 *   1. noise field n [B][H][W] (given, or generated: field 3 of the generator behind cmdax3_randn_fields) -> row pass
 *      r[y][x] = sum_k taps[b][k] * n[y][reflect(x + k - (K-1)/2)];
 *   2. column pass s[y][x] = sum_k taps[b][k] * r[reflect(y + k - (K-1)/2)][x], and per 32 x 32 tile the fp64 sum and sum of squares;
 *   3. mean, unbiased std of s over the sample's H*W pixels (tile partials added in index order, fp64), thr = tf[b] * std + mean (fp32),
 *      out[b][c] = isr[b][c] * (s <= thr ? 1 : 0) for every channel c.
 * reflect is F.pad(mode='reflect'): -i for i < 0, 2(n-1) - i for i >= n.
 * isr, out fp32 [B][C][H][W] (out == isr is allowed); taps fp32 [B][K] (the unnormalised Gaussians of gaussian_kernels); tf fp32 [B]
 * (erfinv(2p - 1) * sqrt 2); field fp32 [B][H][W] or null (then generated from seed, offset + *offset_dev; offset_dev DEVICE int64 or
 * null); enable int32 [B] or null: enable == 0 copies the sample through bit for bit; smooth fp32 [B][H][W] or null: receives s
 * (0 for a gated sample); ws: cmdax4_cow_mask_ws_bytes bytes, 8-byte aligned.
 * CMDA_ERR_SHAPE: B < 0, C < 1, a size < 1, K even, K < 1, K > 255, (K-1)/2 >= min(H, W), B*C*H*W >= 2^31;
 * CMDA_ERR_UNSUPPORTED: null isr / out / taps / tf / ws. */
int cmdax4_cow_mask(const float* isr, float* out, const float* taps, const float* tf, const float* field, const int32_t* enable,
                    float* smooth, void* ws, int B, int C, int H, int W, int K, uint64_t seed, int64_t offset, const int64_t* offset_dev,
                    void* stream);

/* The noise field cmdax4_cow_mask generates for (seed, offset + *offset_dev): out fp32 [B][H][W] = field 3 of the Philox stream of
 * cmdax3_randn_fields (counter word 4 * offset_high + 3; the ISR noise uses fields 0..2), so it is independent of those.
 * CMDA_ERR_SHAPE: B < 0, a size < 1, B*H*W >= 2^31; CMDA_ERR_UNSUPPORTED: null out. */
int cmdax4_cow_field(float* out, int B, int H, int W, uint64_t seed, int64_t offset, const int64_t* offset_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
