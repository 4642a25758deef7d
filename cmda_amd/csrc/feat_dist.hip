// feat_dist.hip -- ImageNet feature-distance loss of DACS (mmseg/models/uda/dacs.py:328-354 calc_feat_dist,
// masked_feat_dist :318-326; mmseg/utils/utils.py:18-39 downscale_label_ratio).
//
// Two launches per step, both deterministic (no float atomics: integer counters and fixed-order sums only):
//   cmda_fdist_label_mask  label [B,H,W] -> rescaled label [B,h,w], mask [B,h,w], count of masked cells (device int32)
//   cmda_fdist_fwd_bwd     student / frozen-encoder stage-4 rows -> loss, per-row norms, gradient ADDED into the student's block
// The cross-workgroup totals (masked-cell count, loss) are taken by the LAST workgroup to finish (an integer ticket in a
// caller-owned int32 that is zero before the launch and zero again after it), summing the per-row partials in index order.
#include "common.h"

namespace {

constexpr int kFdBins = 64;        // classes + the ignore substitute
constexpr int kFdLabelThreads = 256;
constexpr int kFdRowWaves = 4;     // rows per workgroup of the distance kernel (one wave per row)

// Last workgroup of the grid to arrive?  Every thread calls it behind its own stores.  The hand-off is the agent-scope
// release -> integer ticket -> agent-scope acquire form (per-XCD L2s are not coherent): every wave drains its stores, lane 0
// releases, draws a ticket; the last arriver resets the ticket (zero before and after every launch: the caller allocates it
// zeroed once) and acquires before the group reads the other groups' partials.  `flag`: a slot of an existing LDS array.
static __device__ __forceinline__ bool last_group(int* ticket, int* flag) {
#ifndef CMDA_EMU
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  __syncthreads();
  if (threadIdx.x == 0) {
#ifdef CMDA_EMU
    __threadfence();
    const int t = atomicAdd(ticket, 1);
    const bool last = t == (int)gridDim.x - 1;
    if (last) {
      __atomic_store_n(ticket, 0, __ATOMIC_RELAXED);
      __threadfence();
    }
#else
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = t == (int)gridDim.x - 1;
    if (last) {
      __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
#endif
    *flag = last ? 1 : 0;
  }
  __syncthreads();
  const bool last = *flag != 0;
  __syncthreads();   // (the flag's slot is reused by the caller)
  return last;
}

// one workgroup per cell row (b, i): each wave takes cells j = wave, wave + 4, ...; histogram of the s x s block in LDS
// (integer atomics), first-max over the bins (ties -> lowest class), ratio count / (s*s) against min_ratio as avg_pool2d
// computes it; the group's masked-cell count goes to row_counts[b*h + i], the last group sums them into count[0]
__global__ __launch_bounds__(kFdLabelThreads) void fdist_label_kernel(
    const long long* __restrict__ label, int B, int H, int W, int h, int w, int s, int nc, int ignore_index, float min_ratio,
    unsigned class_bits, long long* __restrict__ rescaled, unsigned char* __restrict__ mask, int* __restrict__ row_counts,
    int* __restrict__ count, int* __restrict__ ticket) {
  __shared__ int hist[kFdLabelThreads / 64][kFdBins];
  __shared__ int wave_count[kFdLabelThreads / 64];
  __shared__ int s_sum[kFdLabelThreads];
  const int row = blockIdx.x;   // b * h + i
  const int b = row / h, i = row % h;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nbins = nc + 1;
  int masked = 0;
  constexpr int kWaves = kFdLabelThreads / 64;
  for (int j0 = 0; j0 < w; j0 += kWaves) {   // uniform trip count: every wave meets every barrier
    const int j = j0 + wv;
    for (int k = lane; k < kFdBins; k += 64) hist[wv][k] = 0;
    __syncthreads();
    if (j < w) {
      const long long* base = label + ((long)b * H + (long)i * s) * W + (long)j * s;
      for (int p = lane; p < s * s; p += 64) {
        const int y = p / s, x = p - y * s;
        const long long v = base[(long)y * W + x];
        const int bin = (v >= 0 && v < nc) ? (int)v : nc;   // the ignore index (and anything outside 0..nc-1) -> class nc
        atomicAdd(&hist[wv][bin], 1);
      }
    }
    __syncthreads();
    if (j < w && lane == 0) {
      int best = 0, cnt = hist[wv][0];
      for (int k = 1; k < nbins; ++k)
        if (hist[wv][k] > cnt) { best = k; cnt = hist[wv][k]; }   // first max: ties -> the lowest class
      const float ratio = (float)cnt / (float)(s * s);
      const int out = (best == nc || ratio < min_ratio) ? ignore_index : best;
      const bool in = out >= 0 && out < 32 && ((class_bits >> out) & 1u);
      const long o = (long)row * w + j;
      rescaled[o] = out;
      mask[o] = in ? 1 : 0;
      masked += in ? 1 : 0;
    }
  }
  if (lane == 0) wave_count[wv] = masked;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int k = 0; k < kFdLabelThreads / 64; ++k) t += wave_count[k];
    row_counts[row] = t;
  }
  if (!last_group(ticket, &s_sum[0])) return;
  const int rows = B * h;
  int t = 0;
  for (int r = threadIdx.x; r < rows; r += kFdLabelThreads) t += row_counts[r];
  s_sum[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int k = 0; k < kFdLabelThreads; ++k) tot += s_sum[k];
    count[0] = tot;
  }
}

// V consecutive elements <-> fp32 registers in 16-byte pieces (V = 4 fp32 or 8 bf16 elements per lane and step)
template <int V> static __device__ __forceinline__ void ldv(const float* p, float (&v)[8]) {
#pragma unroll
  for (int k = 0; k < V; k += 4) {
    const float4 t = *reinterpret_cast<const float4*>(p + k);
    v[k] = t.x; v[k + 1] = t.y; v[k + 2] = t.z; v[k + 3] = t.w;
  }
}
template <int V> static __device__ __forceinline__ void stv(float* p, const float (&v)[8]) {
#pragma unroll
  for (int k = 0; k < V; k += 4) *reinterpret_cast<float4*>(p + k) = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
}
template <int V> static __device__ __forceinline__ void ldv(const bf16_t* p, float (&v)[8]) {
  static_assert(V == 8, "bf16 rows move 8 elements per lane and step");
  const u16x8 t = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = bf2f(t[k]);
}
template <int V> static __device__ __forceinline__ void stv(bf16_t* p, const float (&v)[8]) {
  static_assert(V == 8, "bf16 rows move 8 elements per lane and step");
  u16x8 t;
#pragma unroll
  for (int k = 0; k < 8; ++k) t[k] = f2bf(v[k]);
  *reinterpret_cast<u16x8*>(p) = t;
}

// one wave per row: ||fs - ft||_2 over C in fp32 (16-byte loads), norms[r] (0 for rows outside the mask); masked rows with a
// non-zero norm get grad[r] += gscale * lambda / count * d / ||d||.  The last workgroup sums the masked norms in row order:
// loss = lambda * sum / count (NaN when count = 0, as torch.mean of an empty selection).
template <typename T, typename G>
__global__ __launch_bounds__(64 * kFdRowWaves) void fdist_fwd_bwd_kernel(
    const T* __restrict__ fs, const T* __restrict__ ft, const unsigned char* __restrict__ mask, const int* __restrict__ count_ptr,
    int rows, int C, long ldg, float lambda, const float* __restrict__ gscale_ptr, G* __restrict__ grad, float* __restrict__ norms,
    float* __restrict__ loss, int* __restrict__ ticket) {
  constexpr int V = sizeof(T) == 2 ? 8 : 4;
  __shared__ float s_part[64 * kFdRowWaves];
  __shared__ int s_flag[1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = blockIdx.x * kFdRowWaves + wv;
  const int cnt = count_ptr != nullptr ? count_ptr[0] : rows;
  if (r < rows) {
    const bool in = mask == nullptr || mask[r] != 0;
    float nrm = 0.f;
    if (in) {
      const T* a = fs + (long)r * C;
      const T* q = ft + (long)r * C;
      float ss = 0.f;
      for (int c = lane * V; c < C; c += 64 * V) {
        float x[8], y[8];
        ldv<V>(a + c, x);
        ldv<V>(q + c, y);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const float d = x[k] - y[k];
          ss = fmaf(d, d, ss);
        }
      }
      ss = wave_sum(ss);
      nrm = sqrtf(ss);
      if (grad != nullptr && nrm > 0.f && cnt > 0) {
        const float g = gscale_ptr != nullptr ? gscale_ptr[0] : 1.f;
        const float coef = g * lambda / (float)cnt / nrm;
        G* o = grad + (long)r * ldg;
        for (int c = lane * V; c < C; c += 64 * V) {
          float x[8], y[8], z[8];
          ldv<V>(a + c, x);
          ldv<V>(q + c, y);
          ldv<V>(o + c, z);
#pragma unroll
          for (int k = 0; k < V; ++k) z[k] = fmaf(coef, x[k] - y[k], z[k]);
          stv<V>(o + c, z);
        }
      }
    }
    if (lane == 0) norms[r] = nrm;
  }
  if (!last_group(ticket, &s_flag[0])) return;
  float t = 0.f;
  for (int k = threadIdx.x; k < rows; k += 64 * kFdRowWaves) t += norms[k];   // rows outside the mask hold 0
  s_part[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int k = 0; k < 64 * kFdRowWaves; ++k) tot += s_part[k];
    loss[0] = cnt > 0 ? lambda * (tot / (float)cnt) : __builtin_nanf("");
  }
}

}  // namespace

extern "C" int cmda_fdist_label_mask(const int64_t* label, int B, int H, int W, int h, int w, int nc, int ignore_index,
                                     float min_ratio, uint32_t class_bits, int64_t* rescaled, uint8_t* mask, int* row_counts,
                                     int* count, int* ticket, void* stream) {
  if (B <= 0 || h <= 0 || w <= 0) return CMDA_ERR_SHAPE;
  const int s = W / w;
  if (s < 1 || H != h * s || W != w * s) return CMDA_ERR_SHAPE;
  if (nc <= 0 || nc + 1 > kFdBins) return CMDA_ERR_SHAPE;
  if ((long)B * h > 0x7fffffffL) return CMDA_ERR_SHAPE;
  CMDA_LAUNCH(fdist_label_kernel, dim3((unsigned)(B * h)), dim3(kFdLabelThreads), 0, stream, (const long long*)label, B, H, W,
              h, w, s, nc, ignore_index, min_ratio, (unsigned)class_bits, (long long*)rescaled, (unsigned char*)mask, row_counts,
              count, ticket);
  CMDA_CHECK_LAUNCH();
}

extern "C" int cmda_fdist_fwd_bwd(const void* fs, const void* ft, const uint8_t* mask, const int* count, int rows, int C,
                                  int64_t ldg, float lambda, const float* gscale, void* grad, float* norms, float* loss,
                                  int* ticket, int dtype, int grad_dtype, void* stream) {
  if (rows <= 0 || C <= 0) return CMDA_ERR_SHAPE;
  const int v = dtype == CMDA_BF16 ? 8 : 4;
  if (C % v != 0 || (grad != nullptr && (ldg < C || ldg % v != 0))) return CMDA_ERR_SHAPE;
  const dim3 grid((unsigned)((rows + kFdRowWaves - 1) / kFdRowWaves)), block(64 * kFdRowWaves);
#define CMDA_FD_LAUNCH(T, G)                                                                                                  \
  CMDA_LAUNCH((fdist_fwd_bwd_kernel<T, G>), grid, block, 0, stream, (const T*)fs, (const T*)ft, (const unsigned char*)mask, count, \
              rows, C, (long)ldg, lambda, gscale, (G*)grad, norms, loss, ticket)
  if (dtype == CMDA_F32 && grad_dtype == CMDA_F32) CMDA_FD_LAUNCH(float, float);
  else if (dtype == CMDA_BF16 && grad_dtype == CMDA_BF16) CMDA_FD_LAUNCH(bf16_t, bf16_t);
  else if (dtype == CMDA_BF16 && grad_dtype == CMDA_F32) CMDA_FD_LAUNCH(bf16_t, float);
  else return CMDA_ERR_DTYPE;
#undef CMDA_FD_LAUNCH
  CMDA_CHECK_LAUNCH();
}
