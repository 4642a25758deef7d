// ohem.hip -- the OHEM pixel sampler of the decode heads on the device (include/cmda_hip_ext7.h).
//
// Reference:
//   OHEMPixelSampler.sample              mmseg/core/seg/sampler/ohem_pixel_sampler.py:32-78
//   BaseDecodeHead(Fusion).losses        decode_heads/decode_head.py:230-231, :597-598 (seg_weight = sampler.sample(logit, label))
// The reference soft-maxes the full-resolution 19 x H x W logits, gathers the label's probability, compacts the valid pixels, sorts
// ALL of them and reads sort_prob.numel() on the host -- to obtain ONE order statistic and compare every pixel against it.  Here:
//   1. ohem_key_kernel: ce_fwd_kernel's tiling (ce_tile.h: the same up-sampled scores, bit for bit) writes one fp32 key per pixel
//      (probability of the label, or the per-pixel cross-entropy), counts the valid pixels and fills the first histogram;
//   2. an exact most-significant-digit radix select over an order-preserving uint32 image of the keys, 11 / 11 / 10 bits: every
//      workgroup of a pass first redoes the prefix scan of the level before it (2048 counters: 8 per thread, one wave scan), then
//      histograms the next digit of the keys that share the prefix found so far;
//   3. ohem_weight_kernel: scans the last histogram, rebuilds the k-th key's bit pattern and writes the 0/1 weights.
// k comes from n_valid ON THE DEVICE: no host synchronisation, safe inside a captured graph.  All counters are integers (LDS atomics per
// workgroup, one integer global atomic per non-empty bin and workgroup): the result does not depend on scheduling.
#include "ce_tile.h"
#include "../../include/cmda_hip_ext7.h"

namespace {
constexpr int kBins12 = 2048, kBins3 = 1024;           // 11 + 11 + 10 bits
constexpr int kShift1 = 21, kShift2 = 10;
// workspace, in 32-bit words: the state of the select, the three histograms, then the keys
constexpr int kWsValid = 0, kWsBin1 = 1, kWsK1 = 2, kWsPrefix2 = 3, kWsK2 = 4, kWsHist1 = 8, kWsHist2 = kWsHist1 + kBins12,
              kWsHist3 = kWsHist2 + kBins12, kWsCounters = kWsHist3 + kBins3, kWsKeys = (kWsCounters + 3) / 4 * 4;
constexpr unsigned kInvalidBits = 0xFFFFFFFFu;         // key of a pixel that takes no part (a NaN pattern no arithmetic produces)
constexpr int kSelK = 2;                               // `mode` of the stand-alone select: k is read from memory

// fp32 bits -> uint32 with the same order (negative values: all bits flipped; others: the sign bit set)
static __device__ __forceinline__ unsigned ord_of_bits(unsigned u) { return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
static __device__ __forceinline__ unsigned bits_of_ord(unsigned o) { return (o >> 31) ? (o ^ 0x80000000u) : ~o; }

// index (ascending, from 0) of the wanted key among the n_valid keys
static __device__ __forceinline__ unsigned wanted_index(unsigned n_valid, int mode, int batch_kept, const int* __restrict__ k_ptr) {
  if (n_valid == 0) return 0u;
  if (mode == kSelK) return (unsigned)min(max(*k_ptr, 0), (int)n_valid - 1);
  if (mode == CMDAX7_MODE_THRESH) return (unsigned)min(batch_kept, (int)n_valid - 1);   // ohem_pixel_sampler.py:59-60
  return (unsigned)max((int)n_valid - batch_kept, 0);                                   // the batch_kept-th largest
}

// The bin of a histogram of 256 * PER counters that holds the element of index k (ascending), and k's index inside that bin.  Called by
// all 256 threads of the workgroup; sh: 8 words of LDS.  k >= the histogram's total (only when it is empty): bin 0, index 0.
template <int PER>
static __device__ __forceinline__ void find_bin(const unsigned* __restrict__ hist, unsigned k, unsigned* __restrict__ sh, unsigned& bin,
                                                unsigned& krem) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  unsigned c[PER], tot = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    c[j] = hist[threadIdx.x * PER + j];
    tot += c[j];
  }
  unsigned inc = tot;   // inclusive scan over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl(inc, lane >= o ? lane - o : 0, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) sh[wid] = inc;
  if (threadIdx.x == 0) { sh[4] = 0u; sh[5] = 0u; }
  __syncthreads();
  unsigned excl = inc - tot;
  for (int i = 0; i < wid; ++i) excl += sh[i];
  if (k >= excl && k - excl < tot) {   // exactly one thread
    unsigned run = excl;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (k >= run && k - run < c[j]) { sh[4] = (unsigned)(threadIdx.x * PER + j); sh[5] = k - run; }
      run += c[j];
    }
  }
  __syncthreads();
  bin = sh[4];
  krem = sh[5];
}

template <int BINS>
static __device__ __forceinline__ void flush_hist(const unsigned* __restrict__ lds, unsigned* __restrict__ glob) {
  for (int b = threadIdx.x; b < BINS; b += blockDim.x) {
    const unsigned v = lds[b];
    if (v) atomicAdd(glob + b, v);
  }
}

// keys[pix] (bit patterns), ws[kWsValid] += #valid, hist1 += histogram of the valid keys' first digit
__global__ __launch_bounds__(256) void ohem_key_kernel(const float* __restrict__ logits, const long long* __restrict__ label,
                                                        unsigned* __restrict__ keys, unsigned* __restrict__ ws, int B, int h, int w, int H,
                                                        int W, int nc, int ignore_index, int mode) {
  __shared__ float patch[kPatchFloats];
  __shared__ unsigned hist[kBins12];
  __shared__ unsigned nval;
  for (int b = threadIdx.x; b < kBins12; b += 256) hist[b] = 0u;
  if (threadIdx.x == 0) nval = 0u;
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  const ScoreTile t = stage_patch(logits, patch, h, w, H, W, nc, sh, sw);   // (ends in __syncthreads)
  unsigned cnt = 0;
  const int X = t.X0 + (threadIdx.x & (kTW - 1));
  for (int Y = t.Y0 + (threadIdx.x / kTW); Y < min(t.Y0 + kTH, H); Y += 256 / kTW) {
    if (X >= W) break;
    const long i = ((long)t.b * H + Y) * W + X;
    const long long lab = label[i];
    unsigned bits = kInvalidBits;
    if (lab != ignore_index && lab >= 0 && lab < nc) {
      const BilinTap ty = bilin_tap(Y, h, H, sh), tx = bilin_tap(X, w, W, sw);
      float s[kMaxClasses];
      tile_scores<kMaxClasses>(t, logits, patch, h, w, nc, ty, tx, s);
      float mx = -INFINITY;
#pragma unroll
      for (int c = 0; c < kMaxClasses; ++c)
        if (c < nc && s[c] > mx) mx = s[c];
      float se = 0.f;
#pragma unroll
      for (int c = 0; c < kMaxClasses; ++c)
        if (c < nc) se += __expf(s[c] - mx);
      float sl = 0.f;
#pragma unroll
      for (int c = 0; c < kMaxClasses; ++c)
        if (c == (int)lab) sl = s[c];
      // loss: ce_fwd_kernel's lse - score[label]; probability: softmax(scores)[label]
      const float key = mode == CMDAX7_MODE_LOSS ? (mx + __logf(se)) - sl : __expf(sl - mx) / se;
      bits = __float_as_uint(key);
      if (bits == kInvalidBits) bits = 0x7FC00000u;
      atomicAdd(&hist[ord_of_bits(bits) >> kShift1], 1u);
      ++cnt;
    }
    keys[i] = bits;
  }
  if (cnt) atomicAdd(&nval, cnt);
  __syncthreads();
  flush_hist<kBins12>(hist, ws + kWsHist1);
  if (threadIdx.x == 0 && nval) atomicAdd(ws + kWsValid, nval);
}

// the stand-alone select's first pass: every element counts
__global__ __launch_bounds__(256) void select_hist1_kernel(const unsigned* __restrict__ keys, long n, unsigned* __restrict__ ws) {
  __shared__ unsigned hist[kBins12];
  for (int b = threadIdx.x; b < kBins12; b += 256) hist[b] = 0u;
  __syncthreads();
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    atomicAdd(&hist[ord_of_bits(keys[i]) >> kShift1], 1u);
  __syncthreads();
  flush_hist<kBins12>(hist, ws + kWsHist1);
  if (blockIdx.x == 0 && threadIdx.x == 0) ws[kWsValid] = (unsigned)n;   // (the counters were cleared; nothing else writes this word)
}

// LEVEL 2: scan hist1 for the wanted index -> first digit; hist2 += second digit of the keys with that first digit.
// LEVEL 3: scan hist2 -> the first 22 bits; hist3 += last digit of the keys with those 22 bits.
// Workgroup 0 records what its scan found for the next pass (words no workgroup of THIS pass reads).
template <int LEVEL>
__global__ __launch_bounds__(256) void select_refine_kernel(const unsigned* __restrict__ keys, long n, unsigned* __restrict__ ws,
                                                             const int* __restrict__ k_ptr, int mode, int batch_kept, int skip_invalid) {
  __shared__ unsigned hist[kBins12];
  __shared__ unsigned sh[8];
  for (int b = threadIdx.x; b < kBins12; b += 256) hist[b] = 0u;
  unsigned prefix, bin, krem;
  if (LEVEL == 2) {
    const unsigned k = wanted_index(ws[kWsValid], mode, batch_kept, k_ptr);
    find_bin<kBins12 / 256>(ws + kWsHist1, k, sh, bin, krem);
    prefix = bin;
    if (blockIdx.x == 0 && threadIdx.x == 0) { ws[kWsBin1] = prefix; ws[kWsK1] = krem; }
  } else {
    find_bin<kBins12 / 256>(ws + kWsHist2, ws[kWsK1], sh, bin, krem);
    prefix = (ws[kWsBin1] << 11) | bin;
    if (blockIdx.x == 0 && threadIdx.x == 0) { ws[kWsPrefix2] = prefix; ws[kWsK2] = krem; }
  }
  // (find_bin's barriers order the clearing of hist before the atomics below)
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const unsigned bits = keys[i];
    if (skip_invalid && bits == kInvalidBits) continue;
    const unsigned o = ord_of_bits(bits);
    if (LEVEL == 2) {
      if ((o >> kShift1) == prefix) atomicAdd(&hist[(o >> kShift2) & (kBins12 - 1)], 1u);
    } else {
      if ((o >> kShift2) == prefix) atomicAdd(&hist[o & (kBins3 - 1)], 1u);
    }
  }
  __syncthreads();
  if (LEVEL == 2) flush_hist<kBins12>(hist, ws + kWsHist2);
  else flush_hist<kBins3>(hist, ws + kWsHist3);
}

// the bit pattern of the wanted key: the 22 bits found so far and the bin of the last histogram that holds index k2
static __device__ __forceinline__ unsigned kth_bits(const unsigned* __restrict__ ws, unsigned* __restrict__ sh) {
  unsigned bin, krem;
  find_bin<kBins3 / 256>(ws + kWsHist3, ws[kWsK2], sh, bin, krem);
  return bits_of_ord((ws[kWsPrefix2] << 10) | bin);
}

__global__ __launch_bounds__(256) void select_final_kernel(const unsigned* __restrict__ ws, unsigned* __restrict__ out) {
  __shared__ unsigned sh[8];
  const unsigned bits = kth_bits(ws, sh);
  if (threadIdx.x == 0) out[0] = bits;
}

__global__ __launch_bounds__(256) void ohem_weight_kernel(const unsigned* __restrict__ keys, float* __restrict__ weight,
                                                           const unsigned* __restrict__ ws, float* __restrict__ threshold_out, long n,
                                                           int mode, float thresh) {
  __shared__ unsigned sh[8];
  const float kth = __uint_as_float(kth_bits(ws, sh));
  const bool any = ws[kWsValid] != 0u;
  float thr;
  if (mode == CMDAX7_MODE_THRESH) thr = any ? fmaxf(kth, thresh) : thresh;   // ohem_pixel_sampler.py:58-63
  else thr = any ? kth : INFINITY;
  if (threshold_out && blockIdx.x == 0 && threadIdx.x == 0) threshold_out[0] = thr;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const unsigned bits = keys[i];
    const float key = __uint_as_float(bits);
    const bool hard = mode == CMDAX7_MODE_THRESH ? key < thr : key >= thr;
    weight[i] = (bits != kInvalidBits && hard) ? 1.f : 0.f;
  }
}

// workgroups of the passes over the keys: 1024 keys each, at most 1024 workgroups
static inline int pass_grid(long n) { return (int)std::max<long>(1, std::min<long>((n + 1023) / 1024, 1024)); }
}  // namespace

extern "C" int cmdax7_abi_version(void) { return 1; }

extern "C" int64_t cmdax7_ws_bytes(int64_t n_keys) {
  if (n_keys < 0 || n_keys > 0x7fffffffL) return -1;
  return 4 * ((int64_t)kWsKeys + n_keys);
}

extern "C" int cmdax7_select_kth(const float* keys, int64_t n, const int* k, float* out, void* ws, void* stream) {
  if (n < 1 || n > 0x7fffffffL) return CMDA_ERR_SHAPE;
  if (!keys || !k || !out || !ws) return CMDA_ERR_UNSUPPORTED;
  unsigned* w32 = (unsigned*)ws;
  const unsigned* kb = (const unsigned*)keys;
  const int grid = pass_grid(n);
  cmda_zero_async(ws, 4 * (size_t)kWsCounters, stream);
  CMDA_LAUNCH(select_hist1_kernel, dim3(grid), dim3(256), 0, stream, kb, (long)n, w32);
  CMDA_LAUNCH(select_refine_kernel<2>, dim3(grid), dim3(256), 0, stream, kb, (long)n, w32, k, kSelK, 0, 0);
  CMDA_LAUNCH(select_refine_kernel<3>, dim3(grid), dim3(256), 0, stream, kb, (long)n, w32, k, kSelK, 0, 0);
  CMDA_LAUNCH(select_final_kernel, dim3(1), dim3(256), 0, stream, (const unsigned*)w32, (unsigned*)out);
  CMDA_CHECK_LAUNCH();
}

extern "C" int cmdax7_ohem_weight(const float* logits, const int64_t* label, float* weight, float* threshold_out, void* ws, int B, int h,
                                  int w, int H, int W, int nc, int ignore_index, int mode, float thresh, int min_kept, void* stream) {
  if (nc < 1 || nc > kMaxClasses || B < 1 || h < 1 || w < 1 || H < 1 || W < 1 || min_kept < 2) return CMDA_ERR_SHAPE;
  if ((long)B * H * W > 0x7fffffffL) return CMDA_ERR_SHAPE;
  if (!logits || !label || !weight || !ws) return CMDA_ERR_UNSUPPORTED;
  if (mode != CMDAX7_MODE_THRESH && mode != CMDAX7_MODE_LOSS) return CMDA_ERR_UNSUPPORTED;
  const long n = (long)B * H * W;
  const int batch_kept = (int)std::min<long>((long)min_kept * B, 0x7fffffffL);   // (beyond n_valid either way)
  unsigned* w32 = (unsigned*)ws;
  unsigned* keys = w32 + kWsKeys;
  const long tiles = (long)B * ((W + kTW - 1) / kTW) * ((H + kTH - 1) / kTH);   // (<= B*H*W: fits the grid)
  const int grid = pass_grid(n);
  cmda_zero_async(ws, 4 * (size_t)kWsCounters, stream);
  CMDA_LAUNCH(ohem_key_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, logits, (const long long*)label, keys, w32, B, h, w, H, W, nc,
              ignore_index, mode);
  CMDA_LAUNCH(select_refine_kernel<2>, dim3(grid), dim3(256), 0, stream, (const unsigned*)keys, n, w32, (const int*)nullptr, mode,
              batch_kept, 1);
  CMDA_LAUNCH(select_refine_kernel<3>, dim3(grid), dim3(256), 0, stream, (const unsigned*)keys, n, w32, (const int*)nullptr, mode,
              batch_kept, 1);
  CMDA_LAUNCH(ohem_weight_kernel, dim3(grid), dim3(256), 0, stream, (const unsigned*)keys, weight, (const unsigned*)w32, threshold_out, n,
              mode, thresh);
  CMDA_CHECK_LAUNCH();
}
