/* cmda_hip_ext5.h -- fifth extension of the C ABI of libcmda_hip.so: the event tail of the DSEC target loader as batched,
 * bit-reproducible kernels (batched event preparation, an order-preserving voxel grid, a batched events_norm without float atomics).
 *
 * include/cmda_hip.h (version 8) and the tables `cmdax_` .. `cmdax4_` (version 1 each) are frozen; entry points added after them
 * live here under the prefix `cmdax5_`, in the SAME shared library and with the same conventions:
 *  - returns 0 (CMDA_OK) or a negative CMDA_ERR_* code; never throws; a refused call launches nothing and writes nothing; every
 *    refusal is decided on the host before the first launch and before any buffer is touched;
 *  - every pointer is a device pointer unless it says HOST; tensors are contiguous; `void* stream` (a hipStream_t) is the last argument;
 *  - stateless: no allocation, no host synchronisation; no float or double atomics (integer ones only): results are identical from
 *    run to run, bit for bit;
 *  - HOST arrays (sample offsets, clip ranges) are read during the call and travel to the kernels as launch arguments, which is why
 *    a call takes at most CMDAX5_MAX_B samples; the number of launches of a call does not depend on B.
 * A batch of B samples is given as concatenated event arrays and a HOST array offsets[B+1] (int64, non-decreasing): sample b owns
 * the events offsets[b] .. offsets[b+1]-1, N_b = offsets[b+1] - offsets[b] of them; offsets[0] is 0 and n_total = offsets[B].
 * cmdax5_abi_version() versions this table on its own; the versions of the earlier tables are not affected by it.
 */
#ifndef CMDA_HIP_EXT5_H
#define CMDA_HIP_EXT5_H
#include "cmda_hip_ext4.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CMDAX5_MAX_B 256             /* samples of one call (the offsets / clip ranges are launch arguments) */
#define CMDAX5_MAX_EVENTS (1 << 29)  /* a sample holds fewer events than this: an order key is corner * N_b + i + 1 in 32 bits */
#define CMDAX5_SMALL_SEGMENT 32      /* cells with at most this many contributions are ordered by one lane */
#define CMDAX5_SCAN_TILE 2048        /* cells per workgroup of the exclusive scan */
#define CMDAX5_NORM_TILE 2048        /* elements per statistics partial of cmdax5_events_norm_batch (at most 256 partials) */

int cmdax5_abi_version(void);

/* dsec.py:341-353 for B samples in ONE launch: t int64, x / y int32, p uint8 (raw events, concatenated) ->
 * t_norm = (float)(t - t_first) / (float)(t_last - t_first), pol = (float)p and (x, y) = rect_map[y][x] (rect_map fp32 [H][W][2], or
 * null: (float)x, (float)y), each fp32 [n_total].  t_first / t_last are the sample's OWN first and last time stamp, the arithmetic
 * is cmda_event_prep's operation for operation: every sample's slice is bit-identical to a cmda_event_prep call on that sample.
 * A sample with N_b == 0 writes nothing.  x / y are not range-checked against the map (as in cmda_event_prep).
 * CMDA_ERR_SHAPE: B < 1, B > CMDAX5_MAX_B, H or W < 1, offsets[0] != 0, offsets that decrease, a sample with N_b >= 2^29;
 * CMDA_ERR_UNSUPPORTED: a null pointer other than rect_map (the event arrays may be null when n_total == 0). */
int cmdax5_event_prep_batch(const int64_t* t, const int32_t* x, const int32_t* y, const uint8_t* p, const int64_t* offsets /*HOST*/,
                            int B, const float* rect_map, int H, int W, float* t_norm, float* xr, float* yr, float* pol, void* stream);

/* Bytes of the workspace of cmdax5_voxel_ordered, with cells = B*bins*H*W, in this order:
 *     8*(B+1)                                      the offsets on the device (int64)
 *   + 64*n_total                                   one 64-bit record per contribution (order key, weight), eight per event at most
 *   + 4*(cells + 2)                                per cell: contribution count -> segment start -> segment end; the long-cell counter
 *   + 4*B*ceil(bins*H*W / CMDAX5_SCAN_TILE)        scan partials
 *   + 4*(min(cells, 8*n_total / (CMDAX5_SMALL_SEGMENT + 1)) + 1)   list of the cells with more than CMDAX5_SMALL_SEGMENT contributions
 * rounded up to a multiple of 8.  8-byte aligned; contents need no initialisation.
 * 0 for an illegal shape: B < 1, B > CMDAX5_MAX_B, bins / H / W < 1, n_total < 0, cells >= 2^31, n_total > B*(2^29 - 1). */
int64_t cmdax5_voxel_ordered_ws_bytes(int B, int64_t n_total, int bins, int H, int W);

/* events_to_voxel_grid of the reference (mmseg/datasets/dsec.py:26-70) for B samples, ORDER-PRESERVING: t / x / y / pol fp32
 * [n_total] (prepared events, t sorted within a sample), offsets HOST int64 [B+1]; grid fp32 [B][bins][H][W] (every cell is
 * written: no zero-fill needed).
 * Contract: cell (b, tl, yl, xl) = the fp32 sum of the contributions it receives, added ONE AT A TIME starting from 0 in the order
 * (corner pass, event index): corner = 4*ax + 2*ay + at (ax outer, ay, at inner: the eight put_(accumulate=True) calls of the
 * reference in their order), ascending event index inside a pass -- the order of the reference's sequential CPU sum, so the grid is
 * bit-identical to it.  A contribution is cmda_events_to_voxel_grid's, operation for operation with contraction off:
 *   tn = (float)(bins-1) * (t[i] - t[first]) / (t[last] - t[first]);  x0 = (int)x[i], y0 = (int)y[i], tb = (int)tn;
 *   xl = x0 + ax, yl = y0 + ay, tl = tb + at, kept when 0 <= xl < W, 0 <= yl < H, 0 <= tl < bins;
 *   (2*pol[i] - 1) * (1 - |xl - x[i]|) * (1 - |yl - y[i]|) * (1 - |tl - tn|).
 * Eight launches, whatever B: clear the counters, count per cell (integer atomics), exclusive scan per sample (three launches), fill
 * the segments with (order key, weight) records through an integer atomic cursor, sum the short segments (one lane each: repeated
 * selection of the next key), sum the long ones (one workgroup each: an all-ascending bitonic network in LDS up to 4096 records, in
 * the record buffer itself beyond; the weights added by one lane).  A sample with N_b == 0 gives a zero grid.
 * ws: cmdax5_voxel_ordered_ws_bytes(B, offsets[B], bins, H, W) bytes.
 * CMDA_ERR_SHAPE: B < 1, B > CMDAX5_MAX_B, bins / H / W < 1, B*bins*H*W >= 2^31, offsets[0] != 0, offsets that decrease, a sample with
 * N_b >= 2^29;  CMDA_ERR_UNSUPPORTED: a null pointer (the event arrays may be null when n_total == 0). */
int cmdax5_voxel_ordered(const float* t, const float* x, const float* y, const float* pol, const int64_t* offsets /*HOST*/,
                         float* grid, void* ws, int B, int bins, int H, int W, void* stream);

/* Bytes of the workspace of cmdax5_events_norm_batch for B grids of n elements: per grid P = min(256, ceil(n / CMDAX5_NORM_TILE))
 * partials of three doubles (non-zero count, sum, sum of squares), then four uint32 (min / max of the two parts):
 * 24*B*P + 16*B.  0 for B < 1, B > CMDAX5_MAX_B, n < 1 or B*n >= 2^31. */
int64_t cmdax5_events_norm_ws_bytes(int B, int64_t n);

/* events_norm(..., enforce_no_events_zero=True) of the reference (dsec.py:80-121) on each of B grids of n elements, three launches:
 * the statistics of the non-zero standardisation as per-workgroup partials (stored, then added in index order in fp64 by every
 * consumer: a reduction of fixed shape), the min / max of the clipped parts through integer atomics on the bit patterns (order
 * independent), the output.  Per element the arithmetic is cmda_events_norm's.  events, out fp32 [B][n] (out == events is allowed);
 * clip_ranges HOST fp32 [B]; ws: cmdax5_events_norm_ws_bytes(B, n) bytes, 8-byte aligned.
 * CMDA_ERR_SHAPE: B < 1, B > CMDAX5_MAX_B, n < 1, B*n >= 2^31;  CMDA_ERR_UNSUPPORTED: a null pointer. */
int cmdax5_events_norm_batch(const float* events, float* out, void* ws, int B, int64_t n, const float* clip_ranges /*HOST*/,
                             float final_range, void* stream);

#ifdef __cplusplus
}
#endif
#endif
