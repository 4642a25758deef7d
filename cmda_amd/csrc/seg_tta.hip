// seg_tta.hip -- on-device evaluation under test_cfg.mode 'slide' and over several views (multi-scale / flip): the fused
// "per-window up-sample + window sum + divide (+ rescale) + flip-back + {arg-max (+ confusion counters) | soft-max accumulate}" and
// the arg-max of the averaged probabilities.  Entry points of the second ABI extension include/cmda_hip_ext2.h.
//
// Reference:
//   EncoderDecoder.slide_inference / inference / aug_test             segmentors/encoder_decoder.py:175-218, :239-272, :287-304
//     preds = 0; per window (row-major): preds += pad(resize(logits_k -> window)); preds /= count; resize(-> ori_shape) when
//     rescale; softmax; flip back; (aug_test) sum over the views / n; argmax
//
// Like seg_eval.hip no nc x H x W tensor is materialised, per window or per image: a block owns 64 x 8 pixels of the second-stage
// image S2 and each thread rebuilds the class scores of its pixels from the low-resolution logits of the windows that cover them
// with bilin_tap / bilin_mix -- the arithmetic of one cmda_upsample_logits_nchw launch per window, a torch add per window, a divide
// and one more cmda_upsample_logits_nchw launch, bit for bit.  The window grid is a function of six scalars, so the windows that
// cover a pixel are computed, not looked up: per axis they are a run of un-clamped windows (origin i * stride) and possibly the
// last window, the only one the image border can shift back.  Algorithmic bytes per image: K*nc*hl*wl*4 read + OH*OW written
// (labels; + OH*OW*{1,8} ground truth) or nc*OH*OW*4 written (+ as much read when accumulating) (probabilities).
#include "bilinear.h"
#include "../../include/cmda_hip_ext2.h"

namespace {
constexpr int kMaxClasses = CMDAX_MAX_CLASSES;
constexpr int kTW = 64, kTH = 8;   // the tile of seg_eval.hip
constexpr int kChunk = 8;          // classes per pass over a pixel's windows (s1_scores)
constexpr int kMaxBins = (kMaxClasses + 1) * kMaxClasses;

static __device__ __forceinline__ long long load_label(const void* __restrict__ p, int tag, long i) {
  return tag == CMDAX_U8 ? (long long)static_cast<const uint8_t*>(p)[i] : static_cast<const long long*>(p)[i];
}

// conf[k] += hist[k] for the non-zero bins of the block's histogram (seg_eval.hip's counters)
static __device__ __forceinline__ void flush_hist(const unsigned* __restrict__ hist, unsigned long long* __restrict__ conf, int bins) {
  for (int k = threadIdx.x; k < bins; k += blockDim.x) {
    const unsigned v = hist[k];
    if (v) atomicAdd(conf + k, (unsigned long long)v);
  }
}

// One axis of the window grid: `grids` windows of `crop` pixels (crop <= image size), window i < grids - 1 at origin i * stride,
// the last one at `last` = image size - crop (<= (grids - 1) * stride: the only window the border shifts back).
struct WinGrid {
  int crop, stride, grids, last;
};
struct TtaGeo {
  WinGrid y, x;
  int hl, wl, H, W, OH, OW;
};

// the windows that cover pixel p of an axis, in ascending order: `nplain` un-clamped ones from index `lo`, then (n > nplain) the last
struct WinCover {
  int lo, nplain, n;
};
static __device__ __forceinline__ WinCover win_cover(int p, const WinGrid& g) {
  WinCover c;
  c.lo = p >= g.crop ? (p - g.crop) / g.stride + 1 : 0;          // first i with i * stride + crop > p
  c.nplain = max(min(p / g.stride, g.grids - 2) - c.lo + 1, 0);   // last i <= grids - 2 with i * stride <= p
  c.n = c.nplain + (p >= g.last ? 1 : 0);
  return c;
}

// v[k] = S1(y, x) of class c0 + k, k < CH: the window sum in window order (i outer, j inner) from 0, divided by the number of
// windows.  A chunk of CH classes per call keeps CH accumulators and 4 * CH loads in flight instead of 32 and 128 (the kernel's
// registers, and with them its occupancy, are set by these); the taps of a pixel are recomputed per chunk.
template <int CH>
static __device__ __forceinline__ void s1_scores(const float* __restrict__ logits, const TtaGeo& g, int B, int b, int nc, int c0, float sh,
                                                 float sw, int y, int x, float (&v)[CH]) {
#pragma clang fp contract(off)
  const WinCover cy = win_cover(y, g.y), cx = win_cover(x, g.x);
#pragma unroll
  for (int k = 0; k < CH; ++k) v[k] = 0.f;
  for (int iy = 0; iy < cy.n; ++iy) {
    const bool py = iy < cy.nplain;
    const int i = py ? cy.lo + iy : g.y.grids - 1;
    const BilinTap ty = bilin_tap(y - (py ? i * g.y.stride : g.y.last), g.hl, g.y.crop, sh);
    for (int ix = 0; ix < cx.n; ++ix) {
      const bool px = ix < cx.nplain;
      const int j = px ? cx.lo + ix : g.x.grids - 1;
      const BilinTap tx = bilin_tap(x - (px ? j * g.x.stride : g.x.last), g.wl, g.x.crop, sw);
      const float* img = logits + (((long)i * g.x.grids + j) * B + b) * ((long)g.hl * g.wl * nc) + c0;
      const float* r0 = img + (long)ty.i0 * g.wl * nc;
      const float* r1 = img + (long)ty.i1 * g.wl * nc;
      const int a0 = tx.i0 * nc, a1 = tx.i1 * nc;
#pragma unroll
      for (int k = 0; k < CH; ++k)
        if (c0 + k < nc) v[k] = v[k] + bilin_mix(r0[a0 + k], r0[a1 + k], r1[a0 + k], r1[a1 + k], tx.l0, tx.l1, ty.l0, ty.l1);
    }
  }
  const float count = (float)(cy.n * cx.n);
#pragma unroll
  for (int k = 0; k < CH; ++k)
    if (c0 + k < nc) v[k] = v[k] / count;
}

// one row of bilin_mix: bilin_mix(v00, v01, v10, v11, wx0, wx1, wy0, wy1) = bilin_row(v00, v01, wx0, wx1, wy0) +
// bilin_row(v10, v11, wx0, wx1, wy1), every product and sum individually rounded -- the second stage consumes its S1 taps a row at a
// time so that two tap vectors, not four, are live
static __device__ __forceinline__ float bilin_row(float v0, float v1, float wx0, float wx1, float wy) {
#pragma clang fp contract(off)
  const float a = v0 * wx0;
  const float b = v1 * wx1;
  const float row = a + b;
  return row * wy;
}

// grid: B * ceil(OW / 64) * ceil(OH / 8) blocks of 256 threads; tiles are laid out in the frame of S2 (the flipped frame) and the
// output / ground-truth index is the flipped-back one.
template <bool TWO, bool PROB>
__global__ __launch_bounds__(256) void seg_scores_kernel(const float* __restrict__ logits, uint8_t* __restrict__ label_out,
                                                          float* __restrict__ acc, int accumulate, const void* __restrict__ gt,
                                                          int gt_tag, unsigned long long* __restrict__ conf, TtaGeo g, int B, int nc,
                                                          int flip, int ignore_index) {
#pragma clang fp contract(off)
  __shared__ unsigned hist[kMaxBins];
  const int bins = (nc + 1) * nc;
  const bool score = !PROB && conf != nullptr;
  if (score) {
    for (int k = threadIdx.x; k < bins; k += 256) hist[k] = 0u;
    __syncthreads();
  }
  const int OH = g.OH, OW = g.OW;
  const float sh = (float)g.hl / (float)g.y.crop, sw = (float)g.wl / (float)g.x.crop;
  const float sh2 = (float)g.H / (float)OH, sw2 = (float)g.W / (float)OW;
  const int tiles_x = (OW + kTW - 1) / kTW, tiles_y = (OH + kTH - 1) / kTH;
  const int bt = blockIdx.x;
  const int b = bt / (tiles_x * tiles_y);
  const int r = bt - b * tiles_x * tiles_y;
  const int Y0 = (r / tiles_x) * kTH, X0 = (r % tiles_x) * kTW;
  const int Y1 = min(Y0 + kTH, OH) - 1;
  const int X = X0 + (threadIdx.x & (kTW - 1));
  for (int Y = Y0 + (threadIdx.x / kTW); Y <= Y1 && X < OW; Y += 256 / kTW) {
    float s[kMaxClasses];
    const BilinTap y2 = bilin_tap(Y, g.H, OH, sh2), x2 = bilin_tap(X, g.W, OW, sw2);   // (the identity taps when !TWO)
#pragma unroll
    for (int c0 = 0; c0 < kMaxClasses; c0 += kChunk) {   // (unrolled: s[] is indexed by constants)
      if (c0 >= nc) break;
      float p[kChunk], q[kChunk];
      if (!TWO) {
        s1_scores<kChunk>(logits, g, B, b, nc, c0, sh, sw, Y, X, p);
#pragma unroll
        for (int k = 0; k < kChunk; ++k) s[c0 + k] = p[k];
      } else {
        s1_scores<kChunk>(logits, g, B, b, nc, c0, sh, sw, y2.i0, x2.i0, p);
        s1_scores<kChunk>(logits, g, B, b, nc, c0, sh, sw, y2.i0, x2.i1, q);
#pragma unroll
        for (int k = 0; k < kChunk; ++k) s[c0 + k] = bilin_row(p[k], q[k], x2.l0, x2.l1, y2.l0);
        s1_scores<kChunk>(logits, g, B, b, nc, c0, sh, sw, y2.i1, x2.i0, p);
        s1_scores<kChunk>(logits, g, B, b, nc, c0, sh, sw, y2.i1, x2.i1, q);
#pragma unroll
        for (int k = 0; k < kChunk; ++k) s[c0 + k] = s[c0 + k] + bilin_row(p[k], q[k], x2.l0, x2.l1, y2.l1);
      }
    }
    float mx = -INFINITY;
    int am = 0;
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c)
      if (c < nc && s[c] > mx) { mx = s[c]; am = c; }
    const int ox = flip == CMDAX_FLIP_HORIZONTAL ? OW - 1 - X : X, oy = flip == CMDAX_FLIP_VERTICAL ? OH - 1 - Y : Y;
    if (PROB) {
      float se = 0.f;
#pragma unroll
      for (int c = 0; c < kMaxClasses; ++c)
        if (c < nc) { s[c] = expf(s[c] - mx); se += s[c]; }
      const long plane = (long)OH * OW;
      float* a = acc + (long)b * nc * plane + (long)oy * OW + ox;
#pragma unroll
      for (int c = 0; c < kMaxClasses; ++c)
        if (c < nc) {
          const float pr = s[c] / se;
          a[c * plane] = accumulate ? a[c * plane] + pr : pr;
        }
    } else {
      const long o = ((long)b * OH + oy) * OW + ox;
      label_out[o] = (uint8_t)am;
      if (score) {
        const long long gl = load_label(gt, gt_tag, o);
        if (gl != (long long)ignore_index) atomicAdd(&hist[(gl >= 0 && gl < nc ? (int)gl : nc) * nc + am], 1u);
      }
    }
  }
  if (score) {   // (uniform over the block)
    __syncthreads();
    flush_hist(hist, conf, bins);
  }
}

// grid-stride over the B*OH*OW pixels: label = first arg-max over c of acc / n; each block counts into its own LDS histogram
__global__ __launch_bounds__(256) void prob_predict_kernel(const float* __restrict__ acc, uint8_t* __restrict__ label_out,
                                                            const void* __restrict__ gt, int gt_tag,
                                                            unsigned long long* __restrict__ conf, long npix, long plane, int nc, int n,
                                                            int ignore_index) {
  __shared__ unsigned hist[kMaxBins];
  const int bins = (nc + 1) * nc;
  if (conf) {
    for (int k = threadIdx.x; k < bins; k += 256) hist[k] = 0u;
    __syncthreads();
  }
  const float fn = (float)n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long)gridDim.x * 256) {
    const long b = i / plane;
    const float* a = acc + b * nc * plane + (i - b * plane);
    float mx = -INFINITY;
    int am = 0;
    for (int c = 0; c < nc; ++c) {
      const float v = a[c * plane] / fn;
      if (v > mx) { mx = v; am = c; }
    }
    label_out[i] = (uint8_t)am;
    if (conf) {
      const long long gl = load_label(gt, gt_tag, i);
      if (gl != (long long)ignore_index) atomicAdd(&hist[(gl >= 0 && gl < nc ? (int)gl : nc) * nc + am], 1u);
    }
  }
  if (conf) {
    __syncthreads();
    flush_hist(hist, conf, bins);
  }
}

static inline bool label_tag_ok(int tag) { return tag == CMDAX_U8 || tag == CMDAX_I64; }

// one axis of the grid from the reference's scalars; false when the window count leaves 31 bits
static inline bool make_grid(int size, int crop, int stride, WinGrid& g, long& grids) {
  g.crop = std::min(crop, size);
  grids = crop >= size ? 1 : ((long)size - crop + stride - 1) / stride + 1;   // max(size - crop + stride - 1, 0) / stride + 1
  if (grids >= (1L << 31)) return false;
  g.stride = std::min(stride, size);   // (a stride beyond the image: two windows either way, and i * stride stays in range)
  g.grids = (int)grids;
  g.last = size - g.crop;
  return true;
}
}  // namespace

extern "C" int cmdax2_abi_version(void) { return 1; }

extern "C" int cmdax2_seg_scores(const float* logits, int mode, uint8_t* label_out, float* acc, int accumulate, const void* gt,
                                 int gt_dtype, int64_t* conf, int B, int hl, int wl, int H, int W, int crop_h, int crop_w,
                                 int stride_h, int stride_w, int OH, int OW, int nc, int flip, int ignore_index, void* stream) {
  if (nc < 1 || nc > kMaxClasses) return CMDA_ERR_SHAPE;
  if (B < 0 || hl < 1 || wl < 1 || H < 1 || W < 1 || OH < 1 || OW < 1) return CMDA_ERR_SHAPE;
  if (crop_h < 1 || crop_w < 1 || stride_h < 1 || stride_w < 1) return CMDA_ERR_SHAPE;
  TtaGeo g;
  long gy, gx;
  if (!make_grid(H, crop_h, stride_h, g.y, gy) || !make_grid(W, crop_w, stride_w, g.x, gx)) return CMDA_ERR_SHAPE;
  if (gy * gx >= (1L << 31) || gy * gx * B >= (1L << 31)) return CMDA_ERR_SHAPE;
  if ((long)B * OH * OW >= (1L << 31)) return CMDA_ERR_SHAPE;
  if (mode != CMDAX2_LABELS && mode != CMDAX2_PROBS) return CMDA_ERR_UNSUPPORTED;
  if (flip != CMDAX_FLIP_NONE && flip != CMDAX_FLIP_HORIZONTAL && flip != CMDAX_FLIP_VERTICAL) return CMDA_ERR_UNSUPPORTED;
  if ((gt == nullptr) != (conf == nullptr)) return CMDA_ERR_UNSUPPORTED;
  if (mode == CMDAX2_PROBS && (gt != nullptr || acc == nullptr)) return CMDA_ERR_UNSUPPORTED;
  if (mode == CMDAX2_LABELS && label_out == nullptr) return CMDA_ERR_UNSUPPORTED;
  if (gt != nullptr && !label_tag_ok(gt_dtype)) return CMDA_ERR_DTYPE;
  if (B == 0) return CMDA_OK;
  g.hl = hl, g.wl = wl, g.H = H, g.W = W, g.OH = OH, g.OW = OW;
  const long tiles = (long)B * ((OW + kTW - 1) / kTW) * ((OH + kTH - 1) / kTH);   // <= B*OH*OW < 2^31
  const bool two = OH != H || OW != W;
#define CMDA_TTA_LAUNCH(TWO, PROB)                                                                                               \
  CMDA_LAUNCH((seg_scores_kernel<TWO, PROB>), dim3((unsigned)tiles), dim3(256), 0, stream, logits, label_out, acc, accumulate, gt, \
              gt_dtype, (unsigned long long*)conf, g, B, nc, flip, ignore_index)
  if (mode == CMDAX2_PROBS) {
    if (two) CMDA_TTA_LAUNCH(true, true);
    else CMDA_TTA_LAUNCH(false, true);
  } else {
    if (two) CMDA_TTA_LAUNCH(true, false);
    else CMDA_TTA_LAUNCH(false, false);
  }
#undef CMDA_TTA_LAUNCH
  CMDA_CHECK_LAUNCH();
}

extern "C" int cmdax2_prob_predict(const float* acc, uint8_t* label_out, const void* gt, int gt_dtype, int64_t* conf, int B, int OH,
                                   int OW, int nc, int n, int ignore_index, void* stream) {
  if (nc < 1 || nc > kMaxClasses) return CMDA_ERR_SHAPE;
  if (B < 0 || OH < 1 || OW < 1 || n < 1) return CMDA_ERR_SHAPE;
  if ((long)B * OH * OW >= (1L << 31)) return CMDA_ERR_SHAPE;
  if ((gt == nullptr) != (conf == nullptr)) return CMDA_ERR_UNSUPPORTED;
  if (gt != nullptr && !label_tag_ok(gt_dtype)) return CMDA_ERR_DTYPE;
  if (B == 0) return CMDA_OK;
  const long npix = (long)B * OH * OW;
  const int grid = (int)std::max<long>(1, std::min<long>((npix + 1023) / 1024, 4096));
  CMDA_LAUNCH(prob_predict_kernel, dim3(grid), dim3(256), 0, stream, acc, label_out, gt, gt_dtype, (unsigned long long*)conf, npix,
              (long)OH * OW, nc, n, ignore_index);
  CMDA_CHECK_LAUNCH();
}
