// feat_dist.hip -- ImageNet feature-distance loss of DACS (mmseg/models/uda/dacs.py:328-354 calc_feat_dist,
// masked_feat_dist :318-326; mmseg/utils/utils.py:18-39 downscale_label_ratio).
//
// Two launches per step, both deterministic (no float atomics: integer counters and fixed-order sums only):
//   cmda_fdist_label_mask  label [B,H,W] -> rescaled label [B,h,w], mask [B,h,w], count of masked cells (device int32)
//   cmda_fdist_fwd_bwd     student / frozen-encoder stage-4 rows -> loss, per-row norms, gradient ADDED into the student's block
// The cross-workgroup totals (masked-cell count, loss) are taken by the LAST workgroup to finish (an integer ticket in a
// caller-owned int32 that is zero before the launch and zero again after it), summing the per-row partials in index order.
#include "common.h"
#include "../../include/cmda_hip_ext9.h"

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

// ---- feature-consistency loss (include/cmda_hip_ext9.h; encoder_decoder.py:833-848) ---------------------------------------------
// Every level is cut into 16-byte pieces of its rows (V elements; the last piece of a row is short when C % V != 0) and those into
// chunks of kFcThreads * kFcPieces consecutive pieces (kFcPieces per thread, all loads of a chunk in flight at once).  A workgroup
// works on ONE level, chunk wg, wg + nwg, ... of it; the grid is the sum of the levels' workgroups, about kFcGrid in all and shared
// out in proportion to the levels' chunks, so the largest level does not serialise behind a fixed per-level grid.  The grid is kept
// near one workgroup per CU because the arrival ticket is one atomic per workgroup on one address (~22 ns each on the MI355X: at a
// workgroup per chunk, ~500 of them at the step's bf16 sizes, the tickets alone took twice the time of the streaming).
constexpr int kFcThreads = 512;
constexpr int kFcPieces = 4;
constexpr int kFcGrid = 256;

struct FcLevel {
  const void* a;
  const void* b;
  void* g;
  long lda, ldb, ldg;
  unsigned pieces;   // R * ppr
  unsigned ppr;      // pieces per row, ceil(C / V)
  int C;
  int wg0;           // the level's first workgroup
  int nwg;           // the level's workgroups
  int vec;           // base pointers and row strides keep every full piece 16-byte aligned
  float inv_n;       // 1 / (R * C)
};
struct FcArgs {
  FcLevel lv[CMDAX9_MAX_LEVELS];
  int n;
};

// lambda * mean((a - b)^2) per level and its gradient ADDED into the level's block; the modes follow the pointers (loss == nullptr:
// gradient only -- no partial, no ticket; lv.g == nullptr: no gradient for that level).
template <typename T, typename G>
__global__ __launch_bounds__(kFcThreads) void feat_consis_kernel(FcArgs args, float lambda, const float* __restrict__ gscale_ptr,
                                                                float* __restrict__ loss, float* __restrict__ level_loss,
                                                                int* __restrict__ ticket, float* __restrict__ partials) {
  constexpr int V = sizeof(T) == 2 ? 8 : 4;
  __shared__ float s_wave[kFcThreads / 64];
  __shared__ float s_level[CMDAX9_MAX_LEVELS];
  __shared__ int s_flag[1];
  int l = 0;
#pragma unroll
  for (int k = 1; k < CMDAX9_MAX_LEVELS; ++k)
    if (k < args.n && (int)blockIdx.x >= args.lv[k].wg0) l = k;
  const FcLevel& lv = args.lv[l];
  const T* __restrict__ a = (const T*)lv.a;
  const T* __restrict__ b = (const T*)lv.b;
  G* __restrict__ g = (G*)lv.g;
  const float coef = g != nullptr ? (gscale_ptr != nullptr ? gscale_ptr[0] : 1.f) * lambda * (2.f * lv.inv_n) : 0.f;
  constexpr unsigned kChunk = kFcThreads * kFcPieces;
  const unsigned chunks = (lv.pieces + kChunk - 1) / kChunk;
  float ss = 0.f;
  for (unsigned chunk = (unsigned)blockIdx.x - (unsigned)lv.wg0; chunk < chunks; chunk += (unsigned)lv.nwg) {
  const unsigned p0 = chunk * kChunk + threadIdx.x;
  if (lv.vec && lv.C % V == 0) {   // every piece of the level is a full, aligned 16 bytes: the loads of all pieces first
    float x[kFcPieces][8], y[kFcPieces][8];
    long og[kFcPieces];
    bool in[kFcPieces];
#pragma unroll
    for (int k = 0; k < kFcPieces; ++k) {
      const unsigned p = p0 + (unsigned)(k * kFcThreads);
      in[k] = p < lv.pieces;
      const unsigned row = in[k] ? p / lv.ppr : 0u;
      const long col = (long)(in[k] ? p - row * lv.ppr : 0u) * V;
      og[k] = (long)row * lv.ldg + col;
      if (in[k]) {
        ldv<V>(a + ((long)row * lv.lda + col), x[k]);
        ldv<V>(b + ((long)row * lv.ldb + col), y[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < kFcPieces; ++k) {
      if (!in[k]) continue;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        x[k][j] -= y[k][j];
        ss = fmaf(x[k][j], x[k][j], ss);
      }
      if (g != nullptr) {
        float z[8];
        ldv<V>(g + og[k], z);
#pragma unroll
        for (int j = 0; j < V; ++j) z[j] = fmaf(coef, x[k][j], z[j]);
        stv<V>(g + og[k], z);
      }
    }
  } else {
    for (int k = 0; k < kFcPieces; ++k) {
      const unsigned p = p0 + (unsigned)(k * kFcThreads);
      if (p >= lv.pieces) break;
      const unsigned row = p / lv.ppr;
      const int col = (int)(p - row * lv.ppr) * V;
      const T* pa = a + ((long)row * lv.lda + col);
      const T* pb = b + ((long)row * lv.ldb + col);
      G* pg = g != nullptr ? g + ((long)row * lv.ldg + col) : nullptr;
      if (lv.vec && col + V <= lv.C) {
        float x[8], y[8];
        ldv<V>(pa, x);
        ldv<V>(pb, y);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          x[j] -= y[j];
          ss = fmaf(x[j], x[j], ss);
        }
        if (pg != nullptr) {
          float z[8];
          ldv<V>(pg, z);
#pragma unroll
          for (int j = 0; j < V; ++j) z[j] = fmaf(coef, x[j], z[j]);
          stv<V>(pg, z);
        }
      } else {   // the short piece at the end of a row, or a level whose pointers / strides break the alignment
        const int m = lv.C - col < V ? lv.C - col : V;
        for (int j = 0; j < m; ++j) {
          const float d = ldf(pa + j) - ldf(pb + j);
          ss = fmaf(d, d, ss);
          if (pg != nullptr) stf(pg + j, fmaf(coef, d, ldf(pg + j)));
        }
      }
    }
  }
  }
  if (loss == nullptr) return;   // gradient only (uniform over the grid)
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = ss;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int k = 0; k < kFcThreads / 64; ++k) t += s_wave[k];
    partials[blockIdx.x] = t;
  }
  if (!last_group(ticket, &s_flag[0])) return;
  for (int k = 0; k < args.n; ++k) {   // per level: strided sums, butterfly over the wave, the waves in order -- a fixed order
    const int w0 = args.lv[k].wg0, w1 = k + 1 < args.n ? args.lv[k + 1].wg0 : (int)gridDim.x;
    float t = 0.f;
    for (int i = w0 + (int)threadIdx.x; i < w1; i += kFcThreads) t += partials[i];
    t = wave_sum(t);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
      float tot = 0.f;
      for (int i = 0; i < kFcThreads / 64; ++i) tot += s_wave[i];
      s_level[k] = lambda * (tot * args.lv[k].inv_n);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int k = 0; k < args.n; ++k) {
      if (level_loss != nullptr) level_loss[k] = s_level[k];
      tot += s_level[k];
    }
    loss[0] = tot;
  }
}

// host side of cmdax9_*: the shape refusals and the cut of the levels into workgroups (piece: elements per 16 bytes of features)
static int fc_plan(const cmdax9_level_t* levels, int n_levels, int piece, bool strides, FcArgs* out, long* grid) {
  if (n_levels < 1 || n_levels > CMDAX9_MAX_LEVELS) return CMDA_ERR_SHAPE;
  if (levels == nullptr) return CMDA_ERR_UNSUPPORTED;
  long wg = 0, total = 0, chunks[CMDAX9_MAX_LEVELS];
  for (int l = 0; l < n_levels; ++l) {
    const cmdax9_level_t& d = levels[l];
    if (d.R < 1 || d.C < 1) return CMDA_ERR_SHAPE;
    if (strides && (d.lda < d.C || d.ldb < d.C || (d.grad != nullptr && d.ldg < d.C))) return CMDA_ERR_SHAPE;
    const long ppr = ((long)d.C + piece - 1) / piece;
    if (d.R > 0x7fffffffL / ppr) return CMDA_ERR_SHAPE;
    const long pieces = d.R * ppr;
    if (out != nullptr) {
      FcLevel& k = out->lv[l];
      k.a = d.a, k.b = d.b, k.g = d.grad;
      k.lda = d.lda, k.ldb = d.ldb, k.ldg = d.ldg;
      k.pieces = (unsigned)pieces, k.ppr = (unsigned)ppr, k.C = d.C;
      k.inv_n = (float)(1.0 / ((double)d.R * (double)d.C));
    }
    chunks[l] = (pieces + kFcThreads * kFcPieces - 1) / (kFcThreads * kFcPieces);
    total += chunks[l];
  }
  // the levels' shares of about kFcGrid workgroups, at least one each and never more than a level has chunks
  for (int l = 0; l < n_levels; ++l) {
    long n = total <= kFcGrid ? chunks[l] : (chunks[l] * kFcGrid + total - 1) / total;
    n = n < 1 ? 1 : (n > chunks[l] ? chunks[l] : n);
    if (out != nullptr) out->lv[l].wg0 = (int)wg, out->lv[l].nwg = (int)n;
    wg += n;
  }
  if (out != nullptr) out->n = n_levels;
  *grid = wg;
  return CMDA_OK;
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

extern "C" int cmdax9_abi_version(void) { return 1; }

extern "C" int64_t cmdax9_ws_floats(const cmdax9_level_t* levels, int n_levels, int feat_dtype) {
  if (feat_dtype != CMDA_F32 && feat_dtype != CMDA_BF16) return -1;
  long grid = 0;
  return fc_plan(levels, n_levels, feat_dtype == CMDA_BF16 ? 8 : 4, false, nullptr, &grid) == CMDA_OK ? (int64_t)grid : -1;
}

extern "C" int cmdax9_feat_consis(const cmdax9_level_t* levels, int n_levels, float lambda, const float* gscale, float* loss,
                                  float* level_loss, int* ticket, float* partials_ws, int feat_dtype, int grad_dtype, void* stream) {
  FcArgs args;
  long grid = 0;
  const bool tags = (feat_dtype == CMDA_F32 || feat_dtype == CMDA_BF16) && (grad_dtype == CMDA_F32 || grad_dtype == CMDA_BF16);
  const int rc = fc_plan(levels, n_levels, feat_dtype == CMDA_BF16 ? 8 : 4, true, &args, &grid);
  if (rc == CMDA_ERR_SHAPE) return rc;
  if (!tags || (feat_dtype == CMDA_F32 && grad_dtype == CMDA_BF16)) return CMDA_ERR_DTYPE;
  if (rc != CMDA_OK) return rc;
  bool any_grad = false;
  const size_t fsz = feat_dtype == CMDA_BF16 ? 2 : 4, gsz = grad_dtype == CMDA_BF16 ? 2 : 4;
  for (int l = 0; l < n_levels; ++l) {
    FcLevel& k = args.lv[l];
    if (k.a == nullptr || k.b == nullptr) return CMDA_ERR_UNSUPPORTED;
    any_grad = any_grad || k.g != nullptr;
    bool vec = ((uintptr_t)k.a | (uintptr_t)k.b | (uintptr_t)(k.lda * fsz) | (uintptr_t)(k.ldb * fsz)) % 16 == 0;
    if (k.g != nullptr) vec = vec && ((uintptr_t)k.g | (uintptr_t)(k.ldg * gsz)) % 16 == 0;
    k.vec = vec ? 1 : 0;
  }
  if (loss == nullptr && !any_grad) return CMDA_ERR_UNSUPPORTED;
  if (loss != nullptr && (ticket == nullptr || partials_ws == nullptr)) return CMDA_ERR_UNSUPPORTED;
#define CMDA_FC_LAUNCH(T, G)                                                                                              \
  CMDA_LAUNCH((feat_consis_kernel<T, G>), dim3((unsigned)grid), dim3(kFcThreads), 0, stream, args, lambda, gscale, loss, \
              level_loss, ticket, partials_ws)
  if (feat_dtype == CMDA_F32) CMDA_FC_LAUNCH(float, float);
  else if (grad_dtype == CMDA_BF16) CMDA_FC_LAUNCH(bf16_t, bf16_t);
  else CMDA_FC_LAUNCH(bf16_t, float);
#undef CMDA_FC_LAUNCH
  CMDA_CHECK_LAUNCH();
}
