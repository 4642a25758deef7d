// isr_augment.hip -- the ISR augmentations of the night-robustness recipe (third ABI extension, include/cmda_hip_ext3.h):
//   sky mask  (models/utils/dacs_transforms.py:134-171 sky_mask_transform; uda/dacs.py:431-434, datasets/cityscapes_ic.py:303-336)
//   ISR noise (dacs_transforms.py:186-211 add_noise_on_isr; uda/dacs.py:753-755, cityscapes_ic.py:243-261)
// The reference runs both as a per-sample Python loop (three .item() reads, a torch.nonzero sync, a PNG read and a host-side chunk
// shuffle per sample).  Here they are batched launches whose per-sample parameters come from device memory.
//
// Sky mask, three launches:
//   rows : one workgroup per image row -- sky flags -> inclusive prefix sum in LDS -> window count per pixel (<= 61, 6 bits, the sky
//          flag in bit 7) and the row's sky count.  No atomics.
//   cols : one thread per column walks a band of rows down a running sum of the row-window counts: S (<= 3721, sky flag in bit 15);
//          the sample's sky count is the sum of the row counts; max / min of (sky ? 0 : S) by wave reduction and ONE integer atomic
//          pair per workgroup.
//   apply: per pixel, from S and the two integers.
// Integer statistics make the result independent of the order of the workgroups.
#include "bilinear.h"
#include "randn.h"
#include "../../include/cmda_hip_ext3.h"
#include <limits.h>

namespace {

constexpr int kRowThreads = 256;
constexpr int kColThreads = 128;
constexpr int kBand = 16;   // rows per workgroup of the column walk: (k + 2 * kBand) byte reads for kBand outputs

static __device__ __forceinline__ int wave_isum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
static __device__ __forceinline__ int wave_imax(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
static __device__ __forceinline__ int wave_imin(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

static __device__ __forceinline__ int sky_at(const void* label, int tag, long i) {
  return tag == CMDAX_U8 ? (static_cast<const uint8_t*>(label)[i] == CMDAX3_SKY_CLASS)
                         : (static_cast<const long long*>(label)[i] == CMDAX3_SKY_CLASS);
}

static __device__ __forceinline__ bool k_ok(int k) { return k >= 21 && k <= 61 && (k & 1); }

// statistics of sample b: st[4*b + {0 sky count, 1 max, 2 min, 3 unused}]
__global__ void __launch_bounds__(kRowThreads)
sky_rows_kernel(const void* __restrict__ label, int tag, uint8_t* __restrict__ hc, int* __restrict__ rowcnt, int* __restrict__ st,
                const int* __restrict__ prm, const int* __restrict__ enable, int H, int W) {
  __shared__ unsigned short P[CMDAX3_SKY_MAX_W + 1];   // P[x] = sky pixels of the row left of column x
  __shared__ int wsum[kRowThreads / 64];
  const int b = blockIdx.x / H, y = blockIdx.x - b * H;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (y == 0 && t == 0) {
    st[4 * b + 1] = 0;
    st[4 * b + 2] = INT_MAX;
  }
  const int k = prm[4 * b];
  if ((enable != nullptr && enable[b] == 0) || !k_ok(k)) {   // (block-uniform) off: a zero count makes the sample pass through
    if (t == 0) rowcnt[b * H + y] = 0;
    return;
  }
  const long base = ((long)b * H + y) * W;
  const int E = (W + kRowThreads - 1) / kRowThreads;   // consecutive columns per thread
  const int x0 = min(t * E, W), x1 = min(x0 + E, W);
  int s = 0;
  for (int x = x0; x < x1; ++x) s += sky_at(label, tag, base + x);
  int inc = s;   // inclusive scan over the wave, then over the waves
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl(inc, max(lane - o, 0), 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  int run = inc - s;
  for (int i = 0; i < wv; ++i) run += wsum[i];
  if (t == 0) P[0] = 0;
  for (int x = x0; x < x1; ++x) {
    run += sky_at(label, tag, base + x);
    P[x + 1] = (unsigned short)run;
  }
  __syncthreads();
  if (t == 0) rowcnt[b * H + y] = P[W];
  const int r = k >> 1;
  for (int x = t; x < W; x += kRowThreads) {
    const int lo = max(x - r, 0), hi = min(x + r, W - 1);
    const int c = (int)P[hi + 1] - (int)P[lo];
    const int sky = (int)P[x + 1] - (int)P[x];
    hc[base + x] = (uint8_t)(c | (sky << 7));
  }
}

__global__ void __launch_bounds__(kColThreads)
sky_cols_kernel(const uint8_t* __restrict__ hc, const int* __restrict__ rowcnt, int* __restrict__ st, unsigned short* __restrict__ S,
                const int* __restrict__ prm, int H, int W) {
  __shared__ int red[3][kColThreads / 64];
  const int b = blockIdx.z;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  int c = 0;
  for (int i = t; i < H; i += kColThreads) c += rowcnt[b * H + i];
  c = wave_isum(c);
  if (lane == 0) red[0][wv] = c;
  __syncthreads();
  int count = 0;
#pragma unroll
  for (int i = 0; i < kColThreads / 64; ++i) count += red[0][i];
  if (blockIdx.x == 0 && blockIdx.y == 0 && t == 0) st[4 * b] = count;
  if (count < CMDAX3_SKY_MIN_PIXELS) return;   // (block-uniform) the sample passes through: S is not read
  const int r = prm[4 * b] >> 1;                // k is valid here: an invalid k left every row count at zero
  const int x = blockIdx.x * kColThreads + t;
  const int y0 = blockIdx.y * kBand, y1 = min(y0 + kBand, H);
  int mx = 0, mn = INT_MAX;
  if (x < W) {
    const uint8_t* col = hc + (long)b * H * W + x;
    unsigned short* so = S + (long)b * H * W + x;
    int acc = 0;
    for (int yy = max(y0 - r, 0); yy <= min(y0 + r, H - 1); ++yy) acc += col[(long)yy * W] & 63;
    for (int y = y0; y < y1; ++y) {
      const int sky = col[(long)y * W] >> 7;
      so[(long)y * W] = (unsigned short)(acc | (sky << 15));
      const int sm = sky ? 0 : acc;
      mx = max(mx, sm);
      mn = min(mn, sm);
      if (y + 1 + r <= H - 1) acc += col[(long)(y + 1 + r) * W] & 63;
      if (y - r >= 0) acc -= col[(long)(y - r) * W] & 63;
    }
  }
  mx = wave_imax(mx);
  mn = wave_imin(mn);
  if (lane == 0) {
    red[1][wv] = mx;
    red[2][wv] = mn;
  }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int i = 1; i < kColThreads / 64; ++i) {
      mx = max(mx, red[1][i]);
      mn = min(mn, red[2][i]);
    }
    atomicMax(&st[4 * b + 1], mx);
    atomicMin(&st[4 * b + 2], mn);
  }
}

static __device__ __forceinline__ float clamp11(float v) { return fminf(fmaxf(v, -1.f), 1.f); }

// (isr and out may be the same buffer: each pixel is read, then written, by one thread -- no __restrict__ on the two)
__global__ void sky_apply_kernel(const float* isr, const unsigned short* __restrict__ S, const uint8_t* __restrict__ bank,
                                 const int* __restrict__ st, const int* __restrict__ prm, const int* __restrict__ src_row,
                                 const int* __restrict__ src_col, float* out, float* __restrict__ dbg_exp,
                                 float* __restrict__ dbg_bw, int B, int C, int H, int W, int n_bank) {
  const long HW = (long)H * W, total = (long)B * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / HW);
    const long p = i - b * HW;
    const float* src = isr + (long)b * C * HW + p;
    float* dst = out + (long)b * C * HW + p;
    if (st[4 * b] < CMDAX3_SKY_MIN_PIXELS) {
      for (int c = 0; c < C; ++c) dst[c * HW] = src[c * HW];
      if (dbg_exp) dbg_exp[i] = 0.f;
      if (dbg_bw) dbg_bw[i] = 1.f;
      continue;
    }
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    const int k = prm[4 * b];
    const int bi = min(max(prm[4 * b + 1], 0), n_bank - 1);
    const float lam = __int_as_float(prm[4 * b + 2]), inten = __int_as_float(prm[4 * b + 3]);
    const float kk = (float)(k * k);
    const float wmax = (float)st[4 * b + 1] / kk, wmin = (float)st[4 * b + 2] / kk;
    const int s = S[i];
    const int sky = s >> 15, sv = s & 0x7fff;
    const float w = sky ? 0.f : (float)sv / kk;
    const float den = wmax - wmin;
    const float wn = den == 0.f ? 0.f : (w - wmin) / den;
    const float e = wn != 0.f ? wn + lam : wn;   // wn + lambda * (wn != 0)
    const float bw = 1.f - fminf(fmaxf(e, 0.f), 1.f);
    const float ex = sv > 0 ? 1.f : 0.f;
    const int sr = min(max(src_row[b * H + y], 0), H - 1), sc = min(max(src_col[b * W + x], 0), W - 1);
    const float noise = (float)bank[((long)bi * H + sr) * W + sc] / 128.f - 1.f;
    const float keep = sky ? 0.f : 1.f;
    const float add = noise * ex * inten;
    for (int c = 0; c < C; ++c) dst[c * HW] = clamp11(src[c * HW] * keep * bw + add);
    if (dbg_exp) dbg_exp[i] = ex;
    if (dbg_bw) dbg_bw[i] = bw;
  }
}

// ---- counter-based normal fields: randn4 (randn.h) ----------------------------------------------------------------------------
__global__ void randn_fields_kernel(float* __restrict__ out, int B, long HW, unsigned long long seed, long long offset,
                                    const long long* __restrict__ offset_dev) {
  const long Q = (HW + 3) / 4, total = 3 * (long)B * Q;
  const long long off = offset + (offset_dev != nullptr ? *offset_dev : 0);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long fb = i / Q, q = i - fb * Q;
    const int f = (int)(fb / B), b = (int)(fb - (long)f * B);
    float n[4];
    randn4(seed, off, b, f, (unsigned)q, n);
    float* o = out + fb * HW + 4 * q;
    const int np = (int)min(4L, HW - 4 * q);
    for (int j = 0; j < np; ++j) o[j] = n[j];
  }
}

// avg_pool2d(2) at (py, px): the window summed in row-major order, then one division (ATen's loop)
static __device__ __forceinline__ float pool2(const float* __restrict__ pl, int W, int py, int px) {
#pragma clang fp contract(off)
  const float* p = pl + (long)(2 * py) * W + 2 * px;
  float s = p[0];
  s = s + p[1];
  s = s + p[W];
  s = s + p[W + 1];
  return s / 4.f;
}

// Source index and weights of the resize back to H x W.  bilin_tap (bilinear.h) rounds scale * (dst + 0.5) before it subtracts 0.5;
// the ATen builds this is checked against contract the two into one fused multiply-add, and at a non-dyadic scale (odd H or W) the
// two differ by an ulp of the index (~4e-6 at column 70) -- more than the whole error budget of the op.  So the index is fused here,
// explicitly, on both targets; the rest is bilin_tap's guard_index_and_lambda.
static __device__ __forceinline__ BilinTap blur_tap(int dst, int in_size, float scale) {
#pragma clang fp contract(off)
  float real = fmaf(scale, (float)dst + 0.5f, -0.5f);
  if (real < 0.f) real = 0.f;
  int i0 = (int)floorf(real);
  if (i0 > in_size - 1) i0 = in_size - 1;
  const float lam = fminf(fmaxf(real - (float)i0, 0.f), 1.f);
  BilinTap t;
  t.i0 = i0;
  t.i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  t.l1 = lam;
  t.l0 = 1.f - lam;
  return t;
}

template <bool GEN>
__global__ void isr_noise_kernel(const float* __restrict__ isr, float* __restrict__ out, const float* __restrict__ g1,
                                 const float* __restrict__ g2, const float* __restrict__ g3, const int* __restrict__ prm,
                                 const int* __restrict__ enable, int B, int C, int H, int W, int blur, int noise, float scale_h,
                                 float scale_w, unsigned long long seed, long long offset, const long long* __restrict__ offset_dev) {
  const long HW = (long)H * W, Q = (HW + 3) / 4, total = (long)B * Q;
  const int PH = H / 2, PW = W / 2;
  const long long off = offset + (offset_dev != nullptr ? *offset_dev : 0);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / Q);
    const long q = i - b * Q, p0 = 4 * q;
    const int np = (int)min(4L, HW - p0);
    const float* src = isr + (long)b * C * HW;
    float* dst = out + (long)b * C * HW;
    if (enable != nullptr && enable[b] == 0) {
      for (int c = 0; c < C; ++c)
        for (int j = 0; j < np; ++j) dst[c * HW + p0 + j] = src[c * HW + p0 + j];
      continue;
    }
    float f1[4] = {0.f, 0.f, 0.f, 0.f}, f2[4] = {0.f, 0.f, 0.f, 0.f}, f3[4] = {0.f, 0.f, 0.f, 0.f};
    if (noise) {
      if (GEN) {
        randn4(seed, off, b, 0, (unsigned)q, f1);
        randn4(seed, off, b, 1, (unsigned)q, f2);
        randn4(seed, off, b, 2, (unsigned)q, f3);
      } else {
        for (int j = 0; j < np; ++j) {
          f1[j] = g1[(long)b * HW + p0 + j];
          f2[j] = g2[(long)b * HW + p0 + j];
          f3[j] = g3[(long)b * HW + p0 + j];
        }
      }
    }
    const bool blur_b = blur && prm[4 * b] != 0;
    const float t1 = __int_as_float(prm[4 * b + 1]), t2 = __int_as_float(prm[4 * b + 2]), inten = __int_as_float(prm[4 * b + 3]);
    for (int j = 0; j < np; ++j) {
      const long p = p0 + j;
      float v;
      if (blur_b) {
        const int y = (int)(p / W), x = (int)(p - (long)y * W);
        const BilinTap ty = blur_tap(y, PH, scale_h), tx = blur_tap(x, PW, scale_w);
        v = bilin_mix(pool2(src, W, ty.i0, tx.i0), pool2(src, W, ty.i0, tx.i1), pool2(src, W, ty.i1, tx.i0),
                      pool2(src, W, ty.i1, tx.i1), tx.l0, tx.l1, ty.l0, ty.l1);
      } else {
        v = src[p];
      }
      if (noise) {
        v = v * (fabsf(f1[j]) < t1 ? 1.f : 0.f);
        v = v + f3[j] * inten * (fabsf(f2[j]) < t2 ? 1.f : 0.f);
        v = clamp11(v);
      }
      for (int c = 0; c < C; ++c) dst[c * HW + p] = v;
    }
  }
}

static inline int grid_for(long n) { return (int)std::max<long>(1, std::min<long>((n + 255) / 256, 8192)); }

struct SkyWs {
  int* st;
  int* rowcnt;
  unsigned short* S;
  uint8_t* hc;
};
static inline long sky_ws_ints(int B, int H) { return ((long)B * 4 + (long)B * H + 3) / 4 * 4; }
}  // namespace

extern "C" int cmdax3_abi_version(void) { return 1; }

extern "C" int64_t cmdax3_sky_mask_ws_bytes(int B, int H, int W) {
  if (B < 0 || H < 1 || W < 1) return 0;
  return sky_ws_ints(B, H) * 4 + 3 * (int64_t)B * H * W;
}

extern "C" int cmdax3_sky_mask(const void* label, int label_dtype, const float* isr, const uint8_t* bank, const int32_t* prm,
                               const int32_t* src_row, const int32_t* src_col, const int32_t* enable, float* out, float* dbg_expansion,
                               float* dbg_blur_w, void* ws, const int* k_check, int B, int C, int H, int W, int n_bank, int bank_h,
                               int bank_w, void* stream) {
  if (C != 1 && C != 3) return CMDA_ERR_SHAPE;
  if (B < 0 || H < 1 || W < 1 || W > CMDAX3_SKY_MAX_W) return CMDA_ERR_SHAPE;
  if ((long)B * C * H * W >= (1L << 31)) return CMDA_ERR_SHAPE;
  if (n_bank < 1 || bank_h != H || bank_w != W) return CMDA_ERR_SHAPE;
  if (k_check != nullptr)
    for (int b = 0; b < B; ++b)
      if (k_check[b] < 21 || k_check[b] > 61 || !(k_check[b] & 1)) return CMDA_ERR_SHAPE;
  if (label_dtype != CMDAX_U8 && label_dtype != CMDAX_I64) return CMDA_ERR_DTYPE;
  if (!label || !isr || !bank || !prm || !src_row || !src_col || !out || !ws) return CMDA_ERR_UNSUPPORTED;
  if (B == 0) return CMDA_OK;
  SkyWs w;
  w.st = static_cast<int*>(ws);
  w.rowcnt = w.st + 4 * (long)B;
  w.S = reinterpret_cast<unsigned short*>(w.st + sky_ws_ints(B, H));
  w.hc = reinterpret_cast<uint8_t*>(w.S + (long)B * H * W);
  CMDA_LAUNCH(sky_rows_kernel, dim3((unsigned)((long)B * H)), dim3(kRowThreads), 0, stream, label, label_dtype, w.hc, w.rowcnt, w.st,
              prm, enable, H, W);
  CMDA_LAUNCH(sky_cols_kernel, dim3(cdiv(W, kColThreads), cdiv(H, kBand), B), dim3(kColThreads), 0, stream, (const uint8_t*)w.hc,
              (const int*)w.rowcnt, w.st, w.S, prm, H, W);
  CMDA_LAUNCH(sky_apply_kernel, dim3(grid_for((long)B * H * W)), dim3(256), 0, stream, isr, (const unsigned short*)w.S, bank,
              (const int*)w.st, prm, src_row, src_col, out, dbg_expansion, dbg_blur_w, B, C, H, W, n_bank);
  CMDA_CHECK_LAUNCH();
}

extern "C" int cmdax3_randn_fields(float* out, int B, int H, int W, uint64_t seed, int64_t offset, const int64_t* offset_dev,
                                   void* stream) {
  if (B < 0 || H < 1 || W < 1 || (long)B * H * W >= (1L << 31)) return CMDA_ERR_SHAPE;
  if (!out) return CMDA_ERR_UNSUPPORTED;
  if (B == 0) return CMDA_OK;
  const long HW = (long)H * W;
  CMDA_LAUNCH(randn_fields_kernel, dim3(grid_for(3 * (long)B * ((HW + 3) / 4))), dim3(256), 0, stream, out, B, HW,
              (unsigned long long)seed, (long long)offset, (const long long*)offset_dev);
  CMDA_CHECK_LAUNCH();
}

extern "C" int cmdax3_isr_noise(const float* isr, float* out, const float* n1, const float* n2, const float* n3, const int32_t* prm,
                                const int32_t* enable, int B, int C, int H, int W, int blur, int noise, uint64_t seed, int64_t offset,
                                const int64_t* offset_dev, void* stream) {
  if (C != 1 && C != 3) return CMDA_ERR_SHAPE;
  if (B < 0 || H < 1 || W < 1 || (blur && (H < 2 || W < 2))) return CMDA_ERR_SHAPE;
  if ((long)B * C * H * W >= (1L << 31)) return CMDA_ERR_SHAPE;
  if (!isr || !out || !prm || out == isr) return CMDA_ERR_UNSUPPORTED;
  const bool any = n1 || n2 || n3, all = n1 && n2 && n3;
  if (any != all) return CMDA_ERR_UNSUPPORTED;
  if (B == 0) return CMDA_OK;
  const float sh = (float)(H / 2) / (float)H, sw = (float)(W / 2) / (float)W;   // area_pixel_compute_scale: input / output in fp32
  const int grid = grid_for((long)B * (((long)H * W + 3) / 4));
  if (all)
    CMDA_LAUNCH((isr_noise_kernel<false>), dim3(grid), dim3(256), 0, stream, isr, out, n1, n2, n3, prm, enable, B, C, H, W, blur, noise,
                sh, sw, (unsigned long long)seed, (long long)offset, (const long long*)offset_dev);
  else
    CMDA_LAUNCH((isr_noise_kernel<true>), dim3(grid), dim3(256), 0, stream, isr, out, n1, n2, n3, prm, enable, B, C, H, W, blur, noise,
                sh, sw, (unsigned long long)seed, (long long)offset, (const long long*)offset_dev);
  CMDA_CHECK_LAUNCH();
}
