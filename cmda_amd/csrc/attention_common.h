// attention_common.h -- device helpers shared by the fused attention units (attention.hip: head dim 64 and the split-bf16
// instances; attention_wide.hip: head dims 128 ... 1024 walked in 64-wide chunks).  Everything works on [rows][64] bf16 tiles
// in the swizzled LDS layout of load_kv_tile and on the transposed orientation S^T = K Q^T described in attention.hip.
#pragma once
#include "common.h"

namespace {

constexpr int kHD = 64;     // head dim (attention.hip) / width of one head-dim chunk (attention_wide.hip)
constexpr int kMaxK = 256;  // keys kept in LDS (forward and backward)
constexpr int kMaxKFwd = 320;  // ... by the forward-only instance
constexpr int kNT = kMaxK / 16;
constexpr int kKS = 64;        // keys per dK/dV block

// XCD-aware block order: workgroups are dealt round-robin to the 8 XCDs (one L2 each).  All query blocks of one
// (batch, head) read the same K / V, so the 1-D grid is remapped to give each XCD a contiguous band of logical blocks
// (query block fastest): a (batch, head)'s K / V then comes through ONE L2 instead of eight (PMC: 67 MB fetched per
// launch against 17 MB written before this).
static __device__ __forceinline__ unsigned xcd_logical_block() {
  const unsigned nb = gridDim.x, lin = blockIdx.x;
  const unsigned q = nb / 8, r = nb % 8, xcd = lin % 8, loc = lin / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}

// K or V of one (batch, head) -> LDS [kMaxK][64] bf16, 128-byte lines, 16-byte chunk c of line r stored at slot c ^ (r & 7);
// rows >= Nk come from the zero block.  One DMA instruction moves 8 lines (1 KiB); the 4 waves take 8 instructions each.
extern __device__ __attribute__((aligned(16))) unsigned g_attn_zero16[4];
__device__ __attribute__((aligned(16))) unsigned g_attn_zero16[4] = {0u, 0u, 0u, 0u};

template <int MAXK = kMaxK>
static __device__ __forceinline__ void load_kv_tile(const bf16_t* __restrict__ src, int ld, int Nk, bf16_t* lds, int wid,
                                                    int lane, int nwaves) {
  for (int i = wid; i < MAXK / 8; i += nwaves) {
    const int row = 8 * i + (lane >> 3);
    const int chunk = (lane & 7) ^ (row & 7);
    const void* s = row < Nk ? static_cast<const void*>(src + (long)row * ld + chunk * 8)
                             : static_cast<const void*>(g_attn_zero16);
    glds16(s, reinterpret_cast<char*>(lds) + i * 1024);
  }
}

// A operand (rows = 16 consecutive tile rows, k = 32 consecutive d) of a row-major swizzled [rows][64] tile
static __device__ __forceinline__ u16x8 frag_rows(const bf16_t* tile, int row0, int kk, int g, int l15) {
  const int row = row0 + l15;
  return *reinterpret_cast<const u16x8*>(&tile[row * kHD + (((kk * 4 + g) ^ (row & 7)) << 3)]);
}

// A operand of the transposed tile: rows = d (16dt + l15), k slot (g, j) = tile row R0 + j (j < 4) / R1 + (j - 4)
static __device__ __forceinline__ u16x8 frag_cols(const bf16_t* tile, int R0, int R1, int dt, int l15) {
  const int q = l15 >> 2, pp = l15 & 3;
  const int r0 = R0 + q, r1 = R1 + q;
  const int cidx = 2 * dt + (pp >> 1), half = (pp & 1) << 2;
  const u16x4 lo = lds_read_tr16(&tile[r0 * kHD + ((cidx ^ (r0 & 7)) << 3) + half]);
  const u16x4 hi = lds_read_tr16(&tile[r1 * kHD + ((cidx ^ (r1 & 7)) << 3) + half]);
  return u16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

static __device__ __forceinline__ float col_max(float v) {  // over the 4 lane groups holding one query column
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
static __device__ __forceinline__ float col_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// the softmax over keys of raw scores^T p[t][r] = S^T[key 16t + 4g + r][query l15] (scale applied here, keys >= Nk masked)
template <int NT = kNT>
static __device__ __forceinline__ void softmax_keys(int Nk, float scale, int g, f32x4 (&p)[NT], float* lse_out = nullptr) {
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool live = 16 * t + 4 * g + r < Nk;
      p[t][r] = live ? p[t][r] * scale : -INFINITY;
      m = fmaxf(m, p[t][r]);
    }
  m = col_max(m);
  float l = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[t][r] = __expf(p[t][r] - m);  // exp(-inf) = 0 for the masked keys
      l += p[t][r];
    }
  l = col_sum(l);
  if (lse_out) *lse_out = m + __logf(l);
  const float inv = 1.f / l;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) p[t][r] *= inv;
}

// FULL-KEY form (every one of the 16 * NT keys is live, scale > 0): no key mask, no tile guards, and the scale folded into the exponent.
// The max is taken over the RAW scores (scale > 0 keeps the arg-max), e = exp2(s c - m c) with c = scale log2(e) is ONE fma and
// one v_exp_f32 per score, and the probabilities are left UNNORMALISED in p: the callers apply the returned 1 / l to their 16
// output accumulators instead of to 64 probabilities.  lse_out: natural-log log-sum-exp of the SCALED scores, as softmax_keys.
template <int NT = kNT>
static __device__ __forceinline__ float exp_keys_full(float scale, f32x4 (&p)[NT], float* lse_out = nullptr) {
  float m = p[0][0];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) m = fmaxf(m, p[t][r]);
  m = col_max(m);
  const float c = scale * 1.44269504088896340736f, mc = m * c;
  float l = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[t][r] = fast_exp2(fmaf(p[t][r], c, -mc));
      l += p[t][r];
    }
  l = col_sum(l);
  if (lse_out) *lse_out = m * scale + __logf(l);
  return 1.f / l;
}

static __device__ __forceinline__ u16x8 pack_pair(const f32x4& a, const f32x4& b) {
  return u16x8{f2bf(a[0]), f2bf(a[1]), f2bf(a[2]), f2bf(a[3]), f2bf(b[0]), f2bf(b[1]), f2bf(b[2]), f2bf(b[3])};
}

// B operand b[k = d][col = query]: 16 bytes of row (row0 + l15) of a [rows, ld] global matrix; rows past `nrows` repeat the last
static __device__ __forceinline__ void load_qfrag(const bf16_t* __restrict__ base, long row0, long nrows, int ld, int g,
                                                  int l15, u16x8 (&f)[2]) {
  long row = row0 + l15;
  if (row >= nrows) row = nrows - 1;
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) f[kk] = *reinterpret_cast<const u16x8*>(base + row * ld + 32 * kk + 8 * g);
}

}  // namespace

// wide-head instances (attention_wide.hip): head dim C / heads in {128, 192, ..., 1024}; arguments already checked by the C entries
int attn_wide_fwd(const void* q, const void* kv, void* o, int B, int N, int Nk, int heads, int C, float scale, void* stream);
int attn_wide_bwd(const void* q, const void* kv, const void* d_o, void* dq, float* dkv32, float* stats, int B, int N, int Nk,
                  int heads, int C, float scale, void* stream);
