// ce_tile.h -- the tiled "bilinear up-sample of the class scores of one full-resolution pixel" shared by the fused cross-entropy /
// pseudo-label kernels (ce_loss.hip) and the OHEM pixel sampler (ohem.hip): one definition, so that every kernel that scores a pixel
// sees the same bits.
#pragma once
#include "bilinear.h"

namespace {
constexpr int kMaxClasses = 32;

template <int NC_MAX>
static __device__ __forceinline__ void upsample_scores(const float* __restrict__ lg, int b, int h, int w, int nc,
                                                       const BilinTap& ty, const BilinTap& tx, float (&s)[NC_MAX]) {
  const float* p00 = lg + ((long)(b * h + ty.i0) * w + tx.i0) * nc;
  const float* p01 = lg + ((long)(b * h + ty.i0) * w + tx.i1) * nc;
  const float* p10 = lg + ((long)(b * h + ty.i1) * w + tx.i0) * nc;
  const float* p11 = lg + ((long)(b * h + ty.i1) * w + tx.i1) * nc;
#pragma unroll
  for (int c = 0; c < NC_MAX; ++c)
    if (c < nc) s[c] = bilin_mix(p00[c], p01[c], p10[c], p11[c], tx.l0, tx.l1, ty.l0, ty.l1);
}

// Tiled form of the per-pixel kernels: a block owns kTW x kTH full-resolution pixels of one image and first copies the low-resolution
// logits its pixels can touch (a (kTW/scale + 2) x (kTH/scale + 2) patch, 19 floats each: ~4 KB at scale 4) into LDS with coalesced
// loads; the 4 x 19 reads per pixel then come from LDS.  (Straight from global memory every wave-load touched ~16 different
// 76-byte-strided lines: the forward took 62 us for 10 MB, staged 37 us; the pseudo-label kernel 40 -> 23 us; 32-row tiles -- a quarter
// of the same-address atomics -- change nothing.)  Same bilin_mix on the same values: bit-identical scores.
constexpr int kTW = 64, kTH = 8, kPatchFloats = 6144;

struct ScoreTile {
  int X0, Y0, b, tx0, ty0, ncols;
  bool staged;
};

static __device__ __forceinline__ ScoreTile stage_patch(const float* __restrict__ lg, float* __restrict__ patch, int h, int w, int H,
                                                        int W, int nc, float sh, float sw) {
  ScoreTile t;
  const int tiles_x = (W + kTW - 1) / kTW, tiles_y = (H + kTH - 1) / kTH;
  const int bt = blockIdx.x;
  t.b = bt / (tiles_x * tiles_y);
  const int r = bt - t.b * tiles_x * tiles_y;
  t.Y0 = (r / tiles_x) * kTH;
  t.X0 = (r % tiles_x) * kTW;
  const int X1 = min(t.X0 + kTW, W) - 1, Y1 = min(t.Y0 + kTH, H) - 1;
  t.tx0 = bilin_tap(t.X0, w, W, sw).i0;
  t.ty0 = bilin_tap(t.Y0, h, H, sh).i0;
  const int tx1 = bilin_tap(X1, w, W, sw).i1, ty1 = bilin_tap(Y1, h, H, sh).i1;
  t.ncols = tx1 - t.tx0 + 1;
  const int nrows = ty1 - t.ty0 + 1, rowf = t.ncols * nc;
  t.staged = rowf * nrows <= kPatchFloats;
  if (t.staged) {
    for (int rr = 0; rr < nrows; ++rr) {
      const float* src = lg + ((long)(t.b * h + t.ty0 + rr) * w + t.tx0) * nc;
      for (int k = threadIdx.x; k < rowf; k += blockDim.x) patch[rr * rowf + k] = src[k];
    }
  }
  __syncthreads();
  return t;
}

template <int NC_MAX>
static __device__ __forceinline__ void tile_scores(const ScoreTile& t, const float* __restrict__ lg, const float* __restrict__ patch,
                                                   int h, int w, int nc, const BilinTap& ty, const BilinTap& tx, float (&s)[NC_MAX]) {
  if (!t.staged) {
    upsample_scores<NC_MAX>(lg, t.b, h, w, nc, ty, tx, s);
    return;
  }
  const float* p00 = patch + ((ty.i0 - t.ty0) * t.ncols + (tx.i0 - t.tx0)) * nc;
  const float* p01 = patch + ((ty.i0 - t.ty0) * t.ncols + (tx.i1 - t.tx0)) * nc;
  const float* p10 = patch + ((ty.i1 - t.ty0) * t.ncols + (tx.i0 - t.tx0)) * nc;
  const float* p11 = patch + ((ty.i1 - t.ty0) * t.ncols + (tx.i1 - t.tx0)) * nc;
#pragma unroll
  for (int c = 0; c < NC_MAX; ++c)
    if (c < nc) s[c] = bilin_mix(p00[c], p01[c], p10[c], p11[c], tx.l0, tx.l1, ty.l0, ty.l1);
}
}  // namespace
