// seg_eval.hip -- on-device validation: fused "up-sample (+ rescale) + flip-back + arg-max (+ confusion counters)" and the
// confusion counters of label maps that already exist.  Entry points of the ABI extension include/cmda_hip_ext.h.
//
// Reference:
//   FusionEncoderDecoder.whole_inference / inference / simple_test   segmentors/encoder_decoder.py:897-984
//     resize(seg_logit -> input size), resize(-> ori_shape) when rescale, softmax, flip back, argmax
//   intersect_and_union                                               core/evaluation/metrics.py:28-87
//
// Like the teacher's pseudo-label kernel (ce_loss.hip) the nc x H x W logits are never materialised: a block owns 64 x 8 pixels of
// the second-stage image S2, copies the low-resolution logits those pixels can touch THROUGH BOTH bilinear maps into LDS and each
// thread rebuilds the class scores of its pixels with bilin_tap / bilin_mix -- the arithmetic of one or two
// cmda_upsample_logits_nchw launches, bit for bit.  The soft-max is monotone and skipped.  Algorithmic bytes per image:
// nc*h*w*4 read + OH*OW written (+ OH*OW*{1,8} ground truth read); the score is a matrix of integer counters
// conf[(nc+1)][nc] (row = label, row nc = labels out of range but not ignored, column = prediction): a 32-bit LDS histogram per
// block, its non-zero bins flushed with 64-bit integer atomics -- exact, and independent of the order of the blocks.
#include "bilinear.h"
#include "../../include/cmda_hip_ext.h"

namespace {
constexpr int kMaxClasses = CMDAX_MAX_CLASSES;
constexpr int kTW = 64, kTH = 8, kPatchFloats = 6144;   // the tile and LDS budget of ce_loss.hip's tiled kernels
constexpr int kMaxBins = (kMaxClasses + 1) * kMaxClasses;

static __device__ __forceinline__ long long load_label(const void* __restrict__ p, int tag, long i) {
  return tag == CMDAX_U8 ? (long long)static_cast<const uint8_t*>(p)[i] : static_cast<const long long*>(p)[i];
}

// conf[k] += hist[k] for the non-zero bins of the block's histogram
static __device__ __forceinline__ void flush_hist(const unsigned* __restrict__ hist, unsigned long long* __restrict__ conf, int bins) {
  for (int k = threadIdx.x; k < bins; k += blockDim.x) {
    const unsigned v = hist[k];
    if (v) atomicAdd(conf + k, (unsigned long long)v);
  }
}

// Class scores of the S2 pixel (Y, X).  `base` addresses low-resolution pixel (y, x) at base[(y - oy) * rowf + (x - ox) * nc]: the
// LDS patch (origin = its first row / column) or the image itself in global memory (origin 0, rowf = w * nc).
// One stage (S2 = S1): the four low-resolution taps of the pixel.  Two stages: the pixel's four S1 taps, each from its own four
// low-resolution taps, then mixed with the second map's weights -- every S1 value rounded to fp32 as the materialised path stores it.
template <bool TWO>
static __device__ __forceinline__ void seg_scores(const float* __restrict__ base, int rowf, int oy, int ox, int nc, int h, int w, int H,
                                                  int W, int OH, int OW, float sh, float sw, float sh2, float sw2, int Y, int X,
                                                  float (&s)[kMaxClasses]) {
  if (!TWO) {
    const BilinTap ty = bilin_tap(Y, h, H, sh), tx = bilin_tap(X, w, W, sw);
    const float* r0 = base + (ty.i0 - oy) * rowf;
    const float* r1 = base + (ty.i1 - oy) * rowf;
    const int c0 = (tx.i0 - ox) * nc, c1 = (tx.i1 - ox) * nc;
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c)
      if (c < nc) s[c] = bilin_mix(r0[c0 + c], r0[c1 + c], r1[c0 + c], r1[c1 + c], tx.l0, tx.l1, ty.l0, ty.l1);
    return;
  }
  const BilinTap y2 = bilin_tap(Y, H, OH, sh2), x2 = bilin_tap(X, W, OW, sw2);
  const BilinTap ya = bilin_tap(y2.i0, h, H, sh), yb = bilin_tap(y2.i1, h, H, sh);
  const BilinTap xa = bilin_tap(x2.i0, w, W, sw), xb = bilin_tap(x2.i1, w, W, sw);
  const float* ra0 = base + (ya.i0 - oy) * rowf;
  const float* ra1 = base + (ya.i1 - oy) * rowf;
  const float* rb0 = base + (yb.i0 - oy) * rowf;
  const float* rb1 = base + (yb.i1 - oy) * rowf;
  const int ca0 = (xa.i0 - ox) * nc, ca1 = (xa.i1 - ox) * nc, cb0 = (xb.i0 - ox) * nc, cb1 = (xb.i1 - ox) * nc;
#pragma unroll
  for (int c = 0; c < kMaxClasses; ++c) {
    if (c < nc) {
      const float v00 = bilin_mix(ra0[ca0 + c], ra0[ca1 + c], ra1[ca0 + c], ra1[ca1 + c], xa.l0, xa.l1, ya.l0, ya.l1);
      const float v01 = bilin_mix(ra0[cb0 + c], ra0[cb1 + c], ra1[cb0 + c], ra1[cb1 + c], xb.l0, xb.l1, ya.l0, ya.l1);
      const float v10 = bilin_mix(rb0[ca0 + c], rb0[ca1 + c], rb1[ca0 + c], rb1[ca1 + c], xa.l0, xa.l1, yb.l0, yb.l1);
      const float v11 = bilin_mix(rb0[cb0 + c], rb0[cb1 + c], rb1[cb0 + c], rb1[cb1 + c], xb.l0, xb.l1, yb.l0, yb.l1);
      s[c] = bilin_mix(v00, v01, v10, v11, x2.l0, x2.l1, y2.l0, y2.l1);
    }
  }
}

// grid: B * ceil(OW / 64) * ceil(OH / 8) blocks of 256 threads; tiles are laid out in the frame of S2 (the flipped frame) and the
// label / ground-truth index is the flipped-back one.
template <bool TWO>
__global__ __launch_bounds__(256) void seg_predict_kernel(const float* __restrict__ logits, uint8_t* __restrict__ label_out,
                                                           const void* __restrict__ gt, int gt_tag,
                                                           unsigned long long* __restrict__ conf, int B, int h, int w, int H, int W,
                                                           int OH, int OW, int nc, int flip, int ignore_index) {
  __shared__ float patch[kPatchFloats];
  __shared__ unsigned hist[kMaxBins];
  const int bins = (nc + 1) * nc;
  if (conf)
    for (int k = threadIdx.x; k < bins; k += 256) hist[k] = 0u;
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  const float sh2 = (float)H / (float)OH, sw2 = (float)W / (float)OW;
  const int tiles_x = (OW + kTW - 1) / kTW, tiles_y = (OH + kTH - 1) / kTH;
  const int bt = blockIdx.x;
  const int b = bt / (tiles_x * tiles_y);
  const int r = bt - b * tiles_x * tiles_y;
  const int Y0 = (r / tiles_x) * kTH, X0 = (r % tiles_x) * kTW;
  const int X1 = min(X0 + kTW, OW) - 1, Y1 = min(Y0 + kTH, OH) - 1;
  // footprint of the tile: S2 -> S1 (the identity when the sizes agree) -> low resolution; bilin_tap is monotone in its pixel
  const int tx0 = bilin_tap(bilin_tap(X0, W, OW, sw2).i0, w, W, sw).i0, tx1 = bilin_tap(bilin_tap(X1, W, OW, sw2).i1, w, W, sw).i1;
  const int ty0 = bilin_tap(bilin_tap(Y0, H, OH, sh2).i0, h, H, sh).i0, ty1 = bilin_tap(bilin_tap(Y1, H, OH, sh2).i1, h, H, sh).i1;
  const int ncols = tx1 - tx0 + 1, nrows = ty1 - ty0 + 1, rowf = ncols * nc;
  const bool staged = (long)rowf * nrows <= kPatchFloats;
  if (staged) {
    for (int rr = 0; rr < nrows; ++rr) {
      const float* src = logits + ((long)(b * h + ty0 + rr) * w + tx0) * nc;
      for (int k = threadIdx.x; k < rowf; k += 256) patch[rr * rowf + k] = src[k];
    }
  }
  __syncthreads();
  const int X = X0 + (threadIdx.x & (kTW - 1));
  for (int Y = Y0 + (threadIdx.x / kTW); Y <= Y1; Y += 256 / kTW) {
    if (X > X1) break;
    float s[kMaxClasses];
    if (staged)
      seg_scores<TWO>(patch, rowf, ty0, tx0, nc, h, w, H, W, OH, OW, sh, sw, sh2, sw2, Y, X, s);
    else
      seg_scores<TWO>(logits + (long)b * h * w * nc, w * nc, 0, 0, nc, h, w, H, W, OH, OW, sh, sw, sh2, sw2, Y, X, s);
    float mx = -INFINITY;
    int am = 0;
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c)
      if (c < nc && s[c] > mx) { mx = s[c]; am = c; }
    const int ox = flip == CMDAX_FLIP_HORIZONTAL ? OW - 1 - X : X, oy = flip == CMDAX_FLIP_VERTICAL ? OH - 1 - Y : Y;
    const long o = ((long)b * OH + oy) * OW + ox;
    label_out[o] = (uint8_t)am;
    if (conf) {
      const long long g = load_label(gt, gt_tag, o);
      if (g != (long long)ignore_index) atomicAdd(&hist[(g >= 0 && g < nc ? (int)g : nc) * nc + am], 1u);
    }
  }
  if (conf) {   // (uniform over the block)
    __syncthreads();
    flush_hist(hist, conf, bins);
  }
}

// grid-stride over the n pixels; each block counts into its own LDS histogram (at most n / gridDim + 256 < 2^32 per bin)
__global__ __launch_bounds__(256) void confusion_update_kernel(const void* __restrict__ pred, int pred_tag, const void* __restrict__ gt,
                                                                int gt_tag, unsigned long long* __restrict__ conf, long n, int nc,
                                                                int ignore_index) {
  __shared__ unsigned hist[kMaxBins];
  const int bins = (nc + 1) * nc;
  for (int k = threadIdx.x; k < bins; k += 256) hist[k] = 0u;
  __syncthreads();
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long long g = load_label(gt, gt_tag, i), p = load_label(pred, pred_tag, i);
    if (g != (long long)ignore_index && p >= 0 && p < nc) atomicAdd(&hist[(g >= 0 && g < nc ? (int)g : nc) * nc + (int)p], 1u);
  }
  __syncthreads();
  flush_hist(hist, conf, bins);
}

static inline bool label_tag_ok(int tag) { return tag == CMDAX_U8 || tag == CMDAX_I64; }
}  // namespace

extern "C" int cmdax_abi_version(void) { return 1; }

extern "C" int cmdax_seg_predict(const float* logits, uint8_t* label_out, const void* gt, int gt_dtype, int64_t* conf, int B, int h,
                                 int w, int H, int W, int OH, int OW, int nc, int flip, int ignore_index, void* stream) {
  if (nc < 1 || nc > kMaxClasses) return CMDA_ERR_SHAPE;
  if (B < 0 || h < 1 || w < 1 || H < 1 || W < 1 || OH < 1 || OW < 1) return CMDA_ERR_SHAPE;
  if ((long)B * OH * OW >= (1L << 31)) return CMDA_ERR_SHAPE;
  if (flip != CMDAX_FLIP_NONE && flip != CMDAX_FLIP_HORIZONTAL && flip != CMDAX_FLIP_VERTICAL) return CMDA_ERR_UNSUPPORTED;
  if ((gt == nullptr) != (conf == nullptr)) return CMDA_ERR_UNSUPPORTED;
  if (gt != nullptr && !label_tag_ok(gt_dtype)) return CMDA_ERR_DTYPE;
  if (B == 0) return CMDA_OK;
  const long tiles = (long)B * ((OW + kTW - 1) / kTW) * ((OH + kTH - 1) / kTH);   // <= B*OH*OW < 2^31
  if (OH != H || OW != W)
    CMDA_LAUNCH(seg_predict_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, stream, logits, label_out, gt, gt_dtype,
                (unsigned long long*)conf, B, h, w, H, W, OH, OW, nc, flip, ignore_index);
  else
    CMDA_LAUNCH(seg_predict_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, stream, logits, label_out, gt, gt_dtype,
                (unsigned long long*)conf, B, h, w, H, W, OH, OW, nc, flip, ignore_index);
  CMDA_CHECK_LAUNCH();
}

extern "C" int cmdax_confusion_update(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int64_t* conf, int64_t n, int nc,
                                      int ignore_index, void* stream) {
  if (nc < 1 || nc > kMaxClasses) return CMDA_ERR_SHAPE;
  if (n < 0 || n >= (1LL << 40)) return CMDA_ERR_SHAPE;   // (32-bit per-block bins: n / 4096 blocks stays far below 2^32)
  if (!label_tag_ok(pred_dtype) || !label_tag_ok(gt_dtype)) return CMDA_ERR_DTYPE;
  if (n == 0) return CMDA_OK;
  const int grid = (int)std::max<long>(1, std::min<long>((n + 2047) / 2048, 4096));
  CMDA_LAUNCH(confusion_update_kernel, dim3(grid), dim3(256), 0, stream, pred, pred_dtype, gt, gt_dtype, (unsigned long long*)conf,
              (long)n, nc, ignore_index);
  CMDA_CHECK_LAUNCH();
}
