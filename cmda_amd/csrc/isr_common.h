// isr_common.h -- device helpers of the Image Content-Extractor (ISR) shared by extractors.hip (cmda_isr_from_gray) and isr_multi.hip
// (cmdax4_isr_multi).  One definition of the arithmetic, so a channel of the multi-parameter entry point is bit-identical to the
// one-parameter entry point for the same parameters.
#pragma once
#include "common.h"

namespace {

// min/max scratch: per record {min=+inf, max=0, min=+inf, max=0} as float bit patterns (non-negative floats order like uints)
__global__ void minmax_init_kernel(unsigned* __restrict__ mm, int nrec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nrec * 4) mm[i] = (i & 1) ? 0u : 0x7F800000u;
}

static __device__ __forceinline__ float isr_diff(const unsigned char* __restrict__ g, const float* __restrict__ lut,
                                                 int y, int x, int H, int W, int dy, int dx, float thr) {
  // shifted copy with "edge = itself" semantics of np.concatenate in get_image_change_from_pil
  const int sy = y + dy, sx = x + dx;
  const bool inside = sy >= 0 && sy < H && sx >= 0 && sx < W;
  const float front = lut[g[y * W + x]];
  const float now = inside ? lut[g[sy * W + sx]] : front;
  const float d = now - front;
  return fabsf(d) <= thr ? 0.f : d;
}

// One direction's normalised + / - parts of get_ic: m = {pos_min, pos_max, negabs_min, negabs_max} of the whole map.
static __device__ __forceinline__ float isr_norm(float d, float clip, const unsigned* __restrict__ m) {
#pragma clang fp contract(off)
  const float pmin = __uint_as_float(m[0]), pmax = __uint_as_float(m[1]);
  const float namin = __uint_as_float(m[2]), namax = __uint_as_float(m[3]);
  const float pos = fminf(fmaxf(d, 0.f), clip);
  const float neg = fminf(fmaxf(d, -clip), 0.f);
  // tensor_normalize_to_range: (t - tmin) / (tmax - tmin + 1e-8) * (hi - lo) + lo
  const float pn = (pos - pmin) / (pmax - pmin + 1e-8f) * 1.f + 0.f;
  const float nlo = -namax, nhi = -namin;  // min / max of the negative part
  const float nn = (neg - nlo) / (nhi - nlo + 1e-8f) * 1.f + -1.f;
  return pn + nn;
}

}  // namespace
