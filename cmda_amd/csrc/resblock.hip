// resblock.hip -- the tail of the ResNet BasicBlock pairs of ConvertAvgFusion, fused, and its backward (include/cmda_hip_ext8.h).
//
// Reference: mmseg/models/fusion/convert_avg_fusion.py:26-31 -- per feature level (basic_block[2l](f_image) + basic_block[2l+1](f_events)) / 2
// -- and backbones/resnet.py:77-100: out = relu(norm2(conv2(relu(norm1(conv1(x))))) + x).  The convolutions and norm1 run on the
// existing implicit-GEMM / BatchNorm kernels; what is left per level is norm2's apply, the residual add, the ReLU (twice each) and the
// average: composed from the existing kernels ~8 reads and 5 writes of a [M, C] map in 7 launches per level.  Here:
//   forward   out = 0.5 * (relu(bn_i(z_i) + x_i) + relu(bn_e(z_e) + x_e))        4 reads, 1 write, ONE launch for the four levels
//   backward  reduce: s1 = sum g, s2 = sum g xhat per branch, group, channel      5 reads          (g = 0.5 dout [bn(z) + x > 0])
//             apply:  dz = gamma rstd (g - s1/M - xhat s2/M), dres = g            5 reads, 4 writes
// The ReLU masks are recomputed from z, x and the statistics (as bn_bwd_reduce_kernel does): no mask, no per-branch block output is
// stored.  The reduction partials follow batchnorm.hip: 32 slots per (branch, group), then a fold -- which here also adds the sums
// over the groups into dgamma / dbeta (one thread per channel: no atomics there).
//
// One grid serves all levels: the blocks of level l are [start_l, start_{l+1}).  A thread owns V channels -- 4, or 8 with bf16 storage,
// C % 8 == 0 and 16-byte aligned maps (16-byte accesses) -- and a block of 256 threads is TX channel vectors x 256 / TX row lanes, TX
// chosen per level (a power of two that divides C / V where there is one: 8 for the 64-channel level in bf16, so that its 128-byte
// rows fill the wave, 64 for 512 channels); a thread walks its rows 16 / V at a time.
// HBM-bound streaming kernels; fp32 arithmetic.
#include "common.h"
#include "../../include/cmda_hip_ext8.h"

namespace {

constexpr int kSlots = CMDA_BN_SLOTS;

struct LevelK {
  cmdax8_level_t d;
  long ws_off;          // floats: this level's [2 branches][groups][kSlots + 1][2C] inside the workspace
  int start, gx, gy, rpb;   // first block of the level in the streaming grid; channel blocks, row blocks per group, rows per block
  int txl;              // log2 TX: the block is TX channel vectors x (256 >> txl) row lanes
  int fstart, fgx;      // the fold grid: first block, blocks per branch
};
struct Args {
  LevelK lv[CMDAX8_MAX_LEVELS];
  int n, groups;
};

// (static indices only: a level picked with a run-time index would move the descriptors from the kernel-argument segment to scratch)
template <bool kFold>
static __device__ __forceinline__ LevelK pick_level(const Args& a, int bid) {
  LevelK L = a.lv[0];
#pragma unroll
  for (int i = 1; i < CMDAX8_MAX_LEVELS; ++i)
    if (i < a.n && bid >= (kFold ? a.lv[i].fstart : a.lv[i].start)) L = a.lv[i];
  return L;
}

static __device__ __forceinline__ void ldv(const float* p, float (&v)[4]) { ld4(p, v); }
static __device__ __forceinline__ void ldv(const bf16_t* p, float (&v)[4]) { ld4(p, v); }
static __device__ __forceinline__ void stv(float* p, const float (&v)[4]) { st4(p, v); }
static __device__ __forceinline__ void stv(bf16_t* p, const float (&v)[4]) { st4(p, v); }
static __device__ __forceinline__ void ldv(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
static __device__ __forceinline__ void ldv(const bf16_t* p, float (&v)[8]) {
  const u16x8 t = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = bf2f(t[j]);
}
static __device__ __forceinline__ void stv(float* p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
static __device__ __forceinline__ void stv(bf16_t* p, const float (&v)[8]) {
  u16x8 t;
#pragma unroll
  for (int j = 0; j < 8; ++j) t[j] = f2bf(v[j]);
  *reinterpret_cast<u16x8*>(p) = t;
}

// a block's place in its level: channel vector c, rows [r0, r1) of group g
struct Place {
  int c, g, ry, ty;   // ty: row lanes of the block
  long r0, r1, base;   // base: element offset of the group's first row
};
template <int V>
static __device__ __forceinline__ Place place_of(const LevelK& L, int bid) {
  const int local = bid - L.start;
  const int bx = local % L.gx, by = (local / L.gx) % L.gy;
  Place p;
  p.g = local / (L.gx * L.gy);
  p.c = ((bx << L.txl) + (int)(threadIdx.x & ((1u << L.txl) - 1))) * V;
  p.ry = threadIdx.x >> L.txl;
  p.ty = 256 >> L.txl;
  p.r0 = (long)by * L.rpb;
  p.r1 = min((long)L.d.M, p.r0 + L.rpb);
  p.base = (long)p.g * L.d.M * L.d.C;
  return p;
}

// the per-channel constants of one branch in registers
template <int V>
struct BranchConst {
  float mu[V], rs[V], ga[V], be[V];
  __device__ __forceinline__ void load(const cmdax8_branch_t& b, int g, int C, int c) {
    ldv(b.mean + (long)g * C + c, mu);
    ldv(b.rstd + (long)g * C + c, rs);
    ldv(b.gamma + c, ga);
    ldv(b.beta + c, be);
  }
};

template <typename T, int V>
__global__ void __launch_bounds__(256) resavg_fwd_kernel(const Args a) {
  constexpr int U = 16 / V;
  const LevelK L = pick_level<false>(a, blockIdx.x);
  const Place p = place_of<V>(L, blockIdx.x);
  const int C = L.d.C;
  if (p.c >= C) return;
  BranchConst<V> k0, k1;
  k0.load(L.d.br[0], p.g, C, p.c);
  k1.load(L.d.br[1], p.g, C, p.c);
  const T* z0 = (const T*)L.d.br[0].z + p.base + p.c;
  const T* x0 = (const T*)L.d.br[0].x + p.base + p.c;
  const T* z1 = (const T*)L.d.br[1].z + p.base + p.c;
  const T* x1 = (const T*)L.d.br[1].x + p.base + p.c;
  T* out = (T*)L.d.out + p.base + p.c;
  for (long r = p.r0 + p.ry; r < p.r1; r += p.ty * U) {
    float vz0[U][V], vx0[U][V], vz1[U][V], vx1[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long ru = (r + p.ty * u < p.r1 ? r + p.ty * u : r) * C;
      ldv(z0 + ru, vz0[u]);
      ldv(x0 + ru, vx0[u]);
      ldv(z1 + ru, vz1[u]);
      ldv(x1 + ru, vx1[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (r + p.ty * u >= p.r1) break;
      float o[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float a0 = (vz0[u][j] - k0.mu[j]) * k0.rs[j] * k0.ga[j] + k0.be[j] + vx0[u][j];
        const float a1 = (vz1[u][j] - k1.mu[j]) * k1.rs[j] * k1.ga[j] + k1.be[j] + vx1[u][j];
        o[j] = 0.5f * (fmaxf(a0, 0.f) + fmaxf(a1, 0.f));
      }
      stv(out + (r + p.ty * u) * C, o);
    }
  }
}

// ws[level][branch][group][slot][0:C] += sum g, [C:2C] += sum g * xhat
template <typename T, int V>
__global__ void __launch_bounds__(256) resavg_bwd_reduce_kernel(const Args a, float* __restrict__ ws) {
  constexpr int U = 16 / V;
  __shared__ float red[4][256 * V];   // [s1_i, s2_i, s1_e, s2_e][row lane][channel of the block]
  const LevelK L = pick_level<false>(a, blockIdx.x);
  const Place p = place_of<V>(L, blockIdx.x);
  const int C = L.d.C;
  float s[4][V];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int j = 0; j < V; ++j) s[q][j] = 0.f;
  if (p.c < C) {
    BranchConst<V> k0, k1;
    k0.load(L.d.br[0], p.g, C, p.c);
    k1.load(L.d.br[1], p.g, C, p.c);
    const T* z0 = (const T*)L.d.br[0].z + p.base + p.c;
    const T* x0 = (const T*)L.d.br[0].x + p.base + p.c;
    const T* z1 = (const T*)L.d.br[1].z + p.base + p.c;
    const T* x1 = (const T*)L.d.br[1].x + p.base + p.c;
    const T* dout = (const T*)L.d.dout + p.base + p.c;
    for (long r = p.r0 + p.ry; r < p.r1; r += p.ty * U) {
      float vz0[U][V], vx0[U][V], vz1[U][V], vx1[U][V], vd[U][V];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long ru = (r + p.ty * u < p.r1 ? r + p.ty * u : r) * C;
        ldv(z0 + ru, vz0[u]);
        ldv(x0 + ru, vx0[u]);
        ldv(z1 + ru, vz1[u]);
        ldv(x1 + ru, vx1[u]);
        ldv(dout + ru, vd[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (r + p.ty * u >= p.r1) break;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float h = 0.5f * vd[u][j];
          const float xh0 = (vz0[u][j] - k0.mu[j]) * k0.rs[j], xh1 = (vz1[u][j] - k1.mu[j]) * k1.rs[j];
          const float g0 = xh0 * k0.ga[j] + k0.be[j] + vx0[u][j] > 0.f ? h : 0.f;
          const float g1 = xh1 * k1.ga[j] + k1.be[j] + vx1[u][j] > 0.f ? h : 0.f;
          s[0][j] += g0;
          s[1][j] += g0 * xh0;
          s[2][j] += g1;
          s[3][j] += g1 * xh1;
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int j = 0; j < V; ++j) red[q][threadIdx.x * V + j] = s[q][j];   // (thread = ry * TX + cx: row lane major)
  __syncthreads();
  // every thread folds the row lanes of some (sum, channel) pairs: one atomic per channel, sum and block
  const int nch = V << L.txl;   // channels of the block
  const int slot = (int)(p.r0 / L.rpb) % kSlots;
  const int c0 = p.c - (int)(threadIdx.x & ((1u << L.txl) - 1)) * V;   // the block's first channel
  for (int o = threadIdx.x; o < 4 * nch; o += 256) {
    const int q = o / nch, ch = o - q * nch;
    if (c0 + ch >= C) continue;
    float acc = 0.f;
    for (int y = 0; y < p.ty; ++y) acc += red[q][y * nch + ch];
    atomicAdd(ws + L.ws_off + (((long)(q >> 1) * a.groups + p.g) * (kSlots + 1) + slot) * 2 * C + (q & 1) * C + c0 + ch, acc);
  }
}

// the 32 slots of every (level, branch, group) -> slot kSlots; dbeta += sum over the groups of s1, dgamma += ... of s2
__global__ void __launch_bounds__(256) resavg_fold_kernel(const Args a, float* __restrict__ ws) {
  const LevelK L = pick_level<true>(a, blockIdx.x);
  const int local = blockIdx.x - L.fstart;
  const int br = local / L.fgx;
  const int C = L.d.C;
  const int i = (local % L.fgx) * 256 + threadIdx.x;
  if (i >= 2 * C) return;
  float tot = 0.f;
  for (int g = 0; g < a.groups; ++g) {
    float* w = ws + L.ws_off + ((long)br * a.groups + g) * (kSlots + 1) * 2 * C + i;
    float acc = 0.f;
    for (int k = 0; k < kSlots; ++k) acc += w[(long)k * 2 * C];
    w[(long)kSlots * 2 * C] = acc;
    tot += acc;
  }
  float* dbeta = br ? L.d.br[1].dbeta : L.d.br[0].dbeta;   // (static indices: see pick_level)
  float* dgamma = br ? L.d.br[1].dgamma : L.d.br[0].dgamma;
  if (i < C) dbeta[i] += tot;
  else dgamma[i - C] += tot;
}

template <typename T, int V>
__global__ void __launch_bounds__(256) resavg_bwd_apply_kernel(const Args a, const float* __restrict__ ws) {
  constexpr int U = 16 / V;
  const LevelK L = pick_level<false>(a, blockIdx.x);
  const Place p = place_of<V>(L, blockIdx.x);
  const int C = L.d.C;
  if (p.c >= C) return;
  BranchConst<V> k0, k1;
  k0.load(L.d.br[0], p.g, C, p.c);
  k1.load(L.d.br[1], p.g, C, p.c);
  float m[4][V];   // s1_i / M, s2_i / M, s1_e / M, s2_e / M
  const float invM = 1.f / (float)L.d.M;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    ldv(ws + L.ws_off + (((long)(q >> 1) * a.groups + p.g) * (kSlots + 1) + kSlots) * 2 * C + (q & 1) * C + p.c, m[q]);
#pragma unroll
    for (int j = 0; j < V; ++j) m[q][j] *= invM;
  }
  const T* z0 = (const T*)L.d.br[0].z + p.base + p.c;
  const T* x0 = (const T*)L.d.br[0].x + p.base + p.c;
  const T* z1 = (const T*)L.d.br[1].z + p.base + p.c;
  const T* x1 = (const T*)L.d.br[1].x + p.base + p.c;
  const T* dout = (const T*)L.d.dout + p.base + p.c;
  T* dz0 = (T*)L.d.br[0].dz + p.base + p.c;
  T* dr0 = (T*)L.d.br[0].dres + p.base + p.c;
  T* dz1 = (T*)L.d.br[1].dz + p.base + p.c;
  T* dr1 = (T*)L.d.br[1].dres + p.base + p.c;
  for (long r = p.r0 + p.ry; r < p.r1; r += p.ty * U) {
    float vz0[U][V], vx0[U][V], vz1[U][V], vx1[U][V], vd[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long ru = (r + p.ty * u < p.r1 ? r + p.ty * u : r) * C;
      ldv(z0 + ru, vz0[u]);
      ldv(x0 + ru, vx0[u]);
      ldv(z1 + ru, vz1[u]);
      ldv(x1 + ru, vx1[u]);
      ldv(dout + ru, vd[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (r + p.ty * u >= p.r1) break;
      float g0[V], g1[V], d0[V], d1[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float h = 0.5f * vd[u][j];
        const float xh0 = (vz0[u][j] - k0.mu[j]) * k0.rs[j], xh1 = (vz1[u][j] - k1.mu[j]) * k1.rs[j];
        g0[j] = xh0 * k0.ga[j] + k0.be[j] + vx0[u][j] > 0.f ? h : 0.f;
        g1[j] = xh1 * k1.ga[j] + k1.be[j] + vx1[u][j] > 0.f ? h : 0.f;
        d0[j] = k0.ga[j] * k0.rs[j] * (g0[j] - m[0][j] - xh0 * m[1][j]);
        d1[j] = k1.ga[j] * k1.rs[j] * (g1[j] - m[2][j] - xh1 * m[3][j]);
      }
      const long ro = (r + p.ty * u) * C;
      stv(dz0 + ro, d0);
      stv(dr0 + ro, g0);
      stv(dz1 + ro, d1);
      stv(dr1 + ro, g1);
    }
  }
}

// as batchnorm.hip: reductions few fat blocks (one atomic per channel per block), streaming passes >= ~8 blocks per CU -- counted
// over the level alone (the other levels of the launch only add blocks)
static inline int rows_per_block(long rows, int gx, int hi, int lo, int want) {
  int rpb = hi;
  while (rpb > lo && (rows + rpb - 1) / rpb * gx < want) rpb >>= 1;
  return rpb;
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the refusals shared by the three entry points (levels is HOST memory); V = 8 where every map of every level allows 16-byte bf16 rows
static int check_levels(const cmdax8_level_t* levels, int n_levels, int groups) {
  if (n_levels < 1 || n_levels > CMDAX8_MAX_LEVELS || groups < 1 || groups > CMDAX8_MAX_GROUPS) return CMDA_ERR_SHAPE;
  if (!levels) return CMDA_ERR_UNSUPPORTED;
  for (int l = 0; l < n_levels; ++l) {
    const cmdax8_level_t& d = levels[l];
    if (d.C < 4 || (d.C & 3) || d.M < 1) return CMDA_ERR_SHAPE;
    if (d.M > 0x7fffffffL || (long)groups * d.M > 0x7fffffffL / d.C) return CMDA_ERR_SHAPE;   // groups*M*C >= 2^31
  }
  return CMDA_OK;
}

// grid plan; returns the number of streaming blocks.  reduce: the reduction's rows per block, else the streaming passes'
static long plan(Args& a, const cmdax8_level_t* levels, int n_levels, int groups, int V, bool reduce) {
  long blocks = 0, ws = 0;
  int fblocks = 0;
  a.n = n_levels;
  a.groups = groups;
  for (int l = 0; l < n_levels; ++l) {
    LevelK& L = a.lv[l];
    L.d = levels[l];
    const int nvec = L.d.C / V;
    int tx = 64;
    while (tx > 1 && nvec % tx) tx >>= 1;
    if (tx < 8)   // no such divisor: the power of two that covers the row (idle lanes past C), at most 64
      for (tx = 1; tx < nvec && tx < 64;) tx <<= 1;
    for (L.txl = 0; (1 << L.txl) < tx;) ++L.txl;
    L.gx = (nvec + tx - 1) / tx;
    const int sweep = (256 / tx) * (16 / V);   // rows a block covers per iteration: no fewer per block
    L.rpb = reduce ? rows_per_block(L.d.M * groups, L.gx, 512, std::max(32, sweep), 1024)
                   : rows_per_block(L.d.M * groups, L.gx, 256, std::max(16, sweep), 2048);
    L.gy = (int)((L.d.M + L.rpb - 1) / L.rpb);
    L.start = (int)blocks;
    blocks += (long)L.gx * L.gy * groups;
    L.ws_off = ws;
    ws += 2L * groups * (kSlots + 1) * 2 * L.d.C;
    L.fgx = (2 * L.d.C + 255) / 256;
    L.fstart = fblocks;
    fblocks += 2 * L.fgx;
  }
  for (int l = n_levels; l < CMDAX8_MAX_LEVELS; ++l) a.lv[l] = a.lv[0];
  return blocks;
}
}  // namespace

extern "C" int cmdax8_abi_version(void) { return 1; }

extern "C" int64_t cmdax8_ws_floats(const cmdax8_level_t* levels, int n_levels, int groups) {
  if (n_levels < 1 || n_levels > CMDAX8_MAX_LEVELS || groups < 1 || groups > CMDAX8_MAX_GROUPS || !levels) return -1;
  int64_t n = 0;
  for (int l = 0; l < n_levels; ++l) {
    if (levels[l].C < 4 || (levels[l].C & 3)) return -1;
    n += 2L * groups * (kSlots + 1) * 2 * levels[l].C;
  }
  return n;
}

extern "C" int cmdax8_resavg_fwd(const cmdax8_level_t* levels, int n_levels, int groups, int dtype, void* stream) {
  const int rc = check_levels(levels, n_levels, groups);
  if (rc == CMDA_ERR_SHAPE) return rc;
  if (dtype != CMDA_F32 && dtype != CMDA_BF16) return CMDA_ERR_DTYPE;
  if (rc != CMDA_OK) return rc;
  bool wide = dtype == CMDA_BF16;
  for (int l = 0; l < n_levels; ++l) {
    const cmdax8_level_t& d = levels[l];
    if (!d.out) return CMDA_ERR_UNSUPPORTED;
    wide = wide && (d.C & 7) == 0 && aligned16(d.out);
    for (const cmdax8_branch_t& b : d.br) {
      if (!b.z || !b.x || !b.mean || !b.rstd || !b.gamma || !b.beta) return CMDA_ERR_UNSUPPORTED;
      wide = wide && aligned16(b.z) && aligned16(b.x) && aligned16(b.mean) && aligned16(b.rstd) && aligned16(b.gamma) && aligned16(b.beta);
    }
  }
  Args a;
  const long blocks = plan(a, levels, n_levels, groups, wide ? 8 : 4, false);
  if (blocks >= (1L << 31)) return CMDA_ERR_SHAPE;
  if (dtype == CMDA_F32) CMDA_LAUNCH((resavg_fwd_kernel<float, 4>), dim3((unsigned)blocks), dim3(256), 0, stream, a);
  else if (wide) CMDA_LAUNCH((resavg_fwd_kernel<bf16_t, 8>), dim3((unsigned)blocks), dim3(256), 0, stream, a);
  else CMDA_LAUNCH((resavg_fwd_kernel<bf16_t, 4>), dim3((unsigned)blocks), dim3(256), 0, stream, a);
  CMDA_CHECK_LAUNCH();
}

extern "C" int cmdax8_resavg_bwd(const cmdax8_level_t* levels, int n_levels, int groups, float* ws, int dtype, void* stream) {
  const int rc = check_levels(levels, n_levels, groups);
  if (rc == CMDA_ERR_SHAPE) return rc;
  if (dtype != CMDA_F32 && dtype != CMDA_BF16) return CMDA_ERR_DTYPE;
  if (rc != CMDA_OK) return rc;
  if (!ws) return CMDA_ERR_UNSUPPORTED;
  bool wide = dtype == CMDA_BF16 && aligned16(ws);
  for (int l = 0; l < n_levels; ++l) {
    const cmdax8_level_t& d = levels[l];
    if (!d.dout) return CMDA_ERR_UNSUPPORTED;
    wide = wide && (d.C & 7) == 0 && aligned16(d.dout);
    for (const cmdax8_branch_t& b : d.br) {
      if (!b.z || !b.x || !b.mean || !b.rstd || !b.gamma || !b.beta || !b.dz || !b.dres || !b.dgamma || !b.dbeta) return CMDA_ERR_UNSUPPORTED;
      wide = wide && aligned16(b.z) && aligned16(b.x) && aligned16(b.mean) && aligned16(b.rstd) && aligned16(b.gamma) && aligned16(b.beta) &&
             aligned16(b.dz) && aligned16(b.dres);
    }
  }
  const int V = wide ? 8 : 4;
  Args ar, aa;
  const long rblocks = plan(ar, levels, n_levels, groups, V, true);
  const long ablocks = plan(aa, levels, n_levels, groups, V, false);
  if (rblocks >= (1L << 31) || ablocks >= (1L << 31)) return CMDA_ERR_SHAPE;
  const LevelK& last = aa.lv[n_levels - 1];
  cmda_zero_async(ws, sizeof(float) * (size_t)cmdax8_ws_floats(levels, n_levels, groups), stream);
  const dim3 rgrid((unsigned)rblocks), agrid((unsigned)ablocks), fgrid((unsigned)(last.fstart + 2 * last.fgx));
#define CMDAX8_BWD(T, V)                                                                                  \
  do {                                                                                                    \
    CMDA_LAUNCH((resavg_bwd_reduce_kernel<T, V>), rgrid, dim3(256), 0, stream, ar, ws);                   \
    CMDA_LAUNCH(resavg_fold_kernel, fgrid, dim3(256), 0, stream, aa, ws);                                 \
    CMDA_LAUNCH((resavg_bwd_apply_kernel<T, V>), agrid, dim3(256), 0, stream, aa, (const float*)ws);      \
  } while (0)
  if (dtype == CMDA_F32) CMDAX8_BWD(float, 4);
  else if (wide) CMDAX8_BWD(bf16_t, 8);
  else CMDAX8_BWD(bf16_t, 4);
#undef CMDAX8_BWD
  CMDA_CHECK_LAUNCH();
}
