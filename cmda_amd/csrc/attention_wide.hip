// attention_wide.hip -- the fused attention core of attention.hip for WIDE heads: head dim hd = C / heads in {128, 192, ..., 1024}
// (bf16, up to 256 keys; 320 forward-only).  These are the Blocks of the fusion modules, built with num_heads = 1 so that the head
// is the whole channel count (fusion/attention_avg_fusion.py:27-51: 64 / 128 / 320 / 512; fusion/attention_fusion.py:27-59 on the
// concatenated streams: 128 / 256 / 640 / 1024), with the Attention.forward of mix_transformer.py:86-103.
//
// Same orientation as attention.hip (S^T = K Q^T, softmax over keys per lane + two xor-shuffles, P^T reused from the accumulator
// registers as the B operand of the second product); what is new is that the head dim is walked in 64-wide CHUNKS: a chunk of K or V
// is the [keys][64] tile of the head-64 kernels, so every tile helper of attention_common.h applies unchanged.
//   forward      scores accumulate over the hd/64 K chunks (query fragments of the chunk straight from global), softmax, then per
//                V chunk the 64 output columns are computed and stored -- no accumulator lives across chunks.
//   backward dq  scores over the K chunks, dP^T = V dO^T over the V chunks, D, dS^T, then dQ^T per K chunk, stored per chunk.
//   backward dkv a block owns a 64-key slice and 128 queries.  Phase 1: S and dP for its [128][64] corner over the full head dim,
//                operands straight from global (L2), P and dS parked in LDS as bf16 MFMA fragments.  Phase 2: the waves split
//                the 2 hd/64 products dV chunk = P^T dO chunk, dK chunk = dS^T Q chunk (contraction over the 128 queries),
//                each finished in registers and added to dkv32 with one fp32 atomic per element.
// The chunk tiles of the forward-shaped kernels are double-buffered: 2 x 32 KiB at 256 keys, two blocks per CU.
#include "attention_common.h"

namespace {

struct WideParams {
  const bf16_t* q;    // [B*N, C]
  const bf16_t* kv;   // [B*Nk, 2C]
  const bf16_t* d_o;  // [B*N, C]   (backward)
  bf16_t* o;          // [B*N, C]   forward: o; backward: dq
  float* dkv32;       // [B*Nk, 2C] fp32, accumulated
  float* stats;       // [B, heads, N, 2] = (lse, D)
  int B, N, Nk, heads, C, hd;
  float scale;
};

constexpr int kWideQ = 64;  // queries per block of the forward-shaped kernels (4 waves x 16)

// (batch, head, query block) of this workgroup, query block fastest
static __device__ __forceinline__ void wide_block(const WideParams& p, int& b, int& h, long& q0blk) {
  const unsigned nqb = (unsigned)((p.N + kWideQ - 1) / kWideQ);
  const unsigned lb = xcd_logical_block(), bh = lb / nqb;
  q0blk = (long)(lb - bh * nqb) * kWideQ;
  h = (int)(bh % (unsigned)p.heads);
  b = (int)(bh / (unsigned)p.heads);
}

static __device__ __forceinline__ void store_cols(bf16_t* dst, const f32x4 (&acc)[4], int g) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const float v[4] = {acc[dt][0], acc[dt][1], acc[dt][2], acc[dt][3]};
    st4(dst + 16 * dt + 4 * g, v);
  }
}

// acc[dt] = (tile^T x packed)[d = 16 dt + 4g + r][query l15]: the second product of one 64-wide chunk
template <int NT>
static __device__ __forceinline__ void chunk_out(const bf16_t* tile, const u16x8 (&pb)[NT / 2], int nt, int g, int l15, f32x4 (&acc)[4]) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < NT / 2; ++u) {
    if (2 * u < nt) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) acc[dt] = mfma_bf16_16x16x32(frag_cols(tile, 32 * u + 4 * g, 32 * u + 16 + 4 * g, dt, l15), pb[u], acc[dt]);
    }
  }
}

// Tile i of the walk lands in buffer i & 1.  One barrier per tile: in front of it every wave waits for its OWN DMA pieces
// (dma_wait<0>: a wave's vmcnt says nothing about another wave's pieces, and the compiler does not always drain the queue in front
// of a barrier), so behind it tile i has landed as a whole and every wave is done reading tile i - 1, whose buffer then takes
// tile i + 1 while tile i is used.
// PRE(i) requests what tile i needs from global (the query-side fragments) one tile ahead, so that the request is waited for at
// the barrier together with the tile: a global load issued behind the DMA pieces of tile i + 1 and consumed at once would make the
// wave wait for those pieces too (one in-order counter) and serialise the prefetch with the MFMAs.
#define CMDA_WIDE_WALK_ISSUED(ntiles, PRE, ISSUE, USE) /* tile 0 is on its way into s0, PRE(0) done */ \
  for (int i_ = 0; i_ < (ntiles); i_ += 2) {   \
    dma_wait<0>();                             \
    __syncthreads();                           \
    if (i_ + 1 < (ntiles)) ISSUE(i_ + 1, s1);  \
    USE(i_, s0);                               \
    if (i_ + 1 < (ntiles)) {                   \
      PRE(i_ + 1);                             \
      dma_wait<0>();                           \
      __syncthreads();                         \
      if (i_ + 2 < (ntiles)) ISSUE(i_ + 2, s0);\
      USE(i_ + 1, s1);                         \
      PRE(i_ + 2);                             \
    }                                          \
  }
#define CMDA_WIDE_WALK(ntiles, PRE, ISSUE, USE) \
  PRE(0);                                       \
  ISSUE(0, s0);                                 \
  CMDA_WIDE_WALK_ISSUED(ntiles, PRE, ISSUE, USE)

template <int MAXK>
__global__ __launch_bounds__(256, MAXK <= 256 ? 2 : 1) void attn_wide_fwd_kernel(WideParams p) {
  constexpr int NT = MAXK / 16;
  __shared__ __attribute__((aligned(1024))) bf16_t s0[MAXK * kHD];
  __shared__ __attribute__((aligned(1024))) bf16_t s1[MAXK * kHD];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, l15 = lane & 15;
  int b, h;
  long q0;
  wide_block(p, b, h, q0);
  q0 += wid * 16;
  const bool active = q0 < p.N;  // wave-uniform; an idle wave still loads its share of every tile and meets every barrier
  const int nc = p.hd / kHD, nt = (p.Nk + 15) >> 4;
  const bf16_t* kbase = p.kv + (long)b * p.Nk * 2 * p.C + h * p.hd;
  const bf16_t* qb = p.q + (long)b * p.N * p.C + h * p.hd;
  bf16_t* ob = p.o + (long)b * p.N * p.C + h * p.hd;
  f32x4 pr[NT];
  u16x8 pb[NT / 2], qf[2];
#pragma unroll
  for (int t = 0; t < NT; ++t) pr[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // tiles 0 .. nc-1: K chunks, nc .. 2nc-1: V chunks
#define WIDE_PRE(i) if (active && (i) < nc) load_qfrag(qb + (i) * kHD, q0, p.N, p.C, g, l15, qf)
#define WIDE_ISSUE(i, buf) load_kv_tile<MAXK>(kbase + ((i) < nc ? (i) * kHD : p.C + ((i) - nc) * kHD), 2 * p.C, p.Nk, buf, wid, lane, 4)
#define WIDE_USE(i, buf)                                                                                         \
  if (active) {                                                                                                  \
    if ((i) < nc) {                                                                                              \
      _Pragma("unroll") for (int t = 0; t < NT; ++t) {                                                           \
        if (t < nt) {                                                                                            \
          _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                                                       \
            pr[t] = mfma_bf16_16x16x32(frag_rows(buf, 16 * t, kk, g, l15), qf[kk], pr[t]);                       \
        }                                                                                                        \
      }                                                                                                          \
      if ((i) == nc - 1) {                                                                                       \
        softmax_keys<NT>(p.Nk, p.scale, g, pr);                                                                  \
        _Pragma("unroll") for (int u = 0; u < NT / 2; ++u) pb[u] = pack_pair(pr[2 * u], pr[2 * u + 1]);          \
      }                                                                                                          \
    } else {                                                                                                     \
      f32x4 oacc[4];                                                                                             \
      chunk_out<NT>(buf, pb, nt, g, l15, oacc);                                                                  \
      if (q0 + l15 < p.N) store_cols(ob + (q0 + l15) * p.C + ((i) - nc) * kHD, oacc, g);                         \
    }                                                                                                            \
  }
  CMDA_WIDE_WALK(2 * nc, WIDE_PRE, WIDE_ISSUE, WIDE_USE)
#undef WIDE_PRE
#undef WIDE_ISSUE
#undef WIDE_USE
}

// Walk 1 alternates K chunk c (buffer 0: scores) and V chunk c (buffer 1: dP^T); walk 2 takes the K chunks again for dQ^T.  Two loops,
// so that the 128 accumulator registers of P and dP are dead once dS^T is packed (one loop over all 3 hd/64 tiles spilled).
__global__ __launch_bounds__(256, 2) void attn_wide_bwd_dq_kernel(WideParams p) {
  constexpr int NT = kNT;
  __shared__ __attribute__((aligned(1024))) bf16_t s0[kMaxK * kHD];
  __shared__ __attribute__((aligned(1024))) bf16_t s1[kMaxK * kHD];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, l15 = lane & 15;
  int b, h;
  long q0;
  wide_block(p, b, h, q0);
  q0 += wid * 16;
  const bool active = q0 < p.N;  // wave-uniform
  const int nc = p.hd / kHD, nt = (p.Nk + 15) >> 4;
  const bf16_t* kbase = p.kv + (long)b * p.Nk * 2 * p.C + h * p.hd;
  const long rowb = (long)b * p.N;
  const bf16_t* qb = p.q + rowb * p.C + h * p.hd;
  const bf16_t* dob = p.d_o + rowb * p.C + h * p.hd;
  bf16_t* dqb = p.o + rowb * p.C + h * p.hd;
  u16x8 db[NT / 2];
  {
    f32x4 pr[NT], dp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) pr[t] = dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    u16x8 fq[2], fdo[2];  // requested one tile ahead (see CMDA_WIDE_WALK)
    if (active) load_qfrag(qb, q0, p.N, p.C, g, l15, fq);
    load_kv_tile(kbase, 2 * p.C, p.Nk, s0, wid, lane, 4);
    for (int c = 0; c < nc; ++c) {
      dma_wait<0>();
      __syncthreads();  // K chunk c has landed; every wave is done with V chunk c - 1
      load_kv_tile(kbase + p.C + c * kHD, 2 * p.C, p.Nk, s1, wid, lane, 4);
      if (active) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          if (t < nt) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) pr[t] = mfma_bf16_16x16x32(frag_rows(s0, 16 * t, kk, g, l15), fq[kk], pr[t]);
          }
        }
        load_qfrag(dob + c * kHD, q0, p.N, p.C, g, l15, fdo);
      }
      dma_wait<0>();
      __syncthreads();  // V chunk c has landed; every wave is done with K chunk c
      load_kv_tile(kbase + (c + 1 < nc ? (c + 1) * kHD : 0), 2 * p.C, p.Nk, s0, wid, lane, 4);  // the next K chunk, or tile 0 of walk 2
      if (active) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          if (t < nt) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) dp[t] = mfma_bf16_16x16x32(frag_rows(s1, 16 * t, kk, g, l15), fdo[kk], dp[t]);
          }
        }
        if (c + 1 < nc) load_qfrag(qb + (c + 1) * kHD, q0, p.N, p.C, g, l15, fq);
      }
    }
    if (active) {
      float lse;
      softmax_keys<NT>(p.Nk, p.scale, g, pr, &lse);
      float dsum = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) dsum += pr[t][r] * dp[t][r];
      dsum = col_sum(dsum);
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) dp[t][r] = p.scale * pr[t][r] * (dp[t][r] - dsum);  // dS^T
#pragma unroll
      for (int u = 0; u < NT / 2; ++u) db[u] = pack_pair(dp[2 * u], dp[2 * u + 1]);
      if (g == 0 && q0 + l15 < p.N) {
        float* st = p.stats + ((long)b * p.heads + h) * p.N * 2;
        st[(q0 + l15) * 2 + 0] = lse;
        st[(q0 + l15) * 2 + 1] = dsum;
      }
    }
  }
#define WIDE_ISSUE(i, buf) load_kv_tile(kbase + (i) * kHD, 2 * p.C, p.Nk, buf, wid, lane, 4)
#define WIDE_USE(i, buf)                                                                      \
  if (active) {                                                                               \
    f32x4 dqacc[4];                                                                           \
    chunk_out<NT>(buf, db, nt, g, l15, dqacc);                                                \
    if (q0 + l15 < p.N) store_cols(dqb + (q0 + l15) * p.C + (i) * kHD, dqacc, g);             \
  }
#define WIDE_PRE(i)
  CMDA_WIDE_WALK_ISSUED(nc, WIDE_PRE, WIDE_ISSUE, WIDE_USE)
#undef WIDE_PRE
#undef WIDE_ISSUE
#undef WIDE_USE
}

// ---- dK | dV
constexpr int kSpanQ = 128;  // queries per block: 4 waves x 32 in phase 1, four 32-query tiles per product in phase 2

// 16 bytes (d = 32 kk + 8 g ...) of row min(row, last) of a [rows, ld] global matrix: the A or B fragment of one 16 x 32 corner
static __device__ __forceinline__ u16x8 gfrag(const bf16_t* __restrict__ base, long row, long last, long ld, int kk, int g) {
  return *reinterpret_cast<const u16x8*>(base + (row < last ? row : last) * ld + 32 * kk + 8 * g);
}

__global__ __launch_bounds__(256, 2) void attn_wide_bwd_dkv_kernel(WideParams p) {
  // parked fragments: [32-query tile][key tile][lane] x 16 bytes -- exactly what pack_pair hands the MFMA, read back by the same lane id
  __shared__ __attribute__((aligned(16))) u16x8 sP[4 * 4 * 64];
  __shared__ __attribute__((aligned(16))) u16x8 sDS[4 * 4 * 64];
  __shared__ __attribute__((aligned(1024))) bf16_t sStage[4 * 2 * 32 * kHD];  // per wave: two 32 x 64 tiles of dO or Q (double buffer)
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, l15 = lane & 15;
  // logical order: key slice fastest (the four slices of one (batch, head, span) read the same Q / dO rows), then span
  const unsigned lb = xcd_logical_block();
  const int ks = (int)(lb & 3);
  const unsigned spans = (unsigned)((p.N + kSpanQ - 1) / kSpanQ);
  const unsigned span = (lb >> 2) % spans, bh = (lb >> 2) / spans;
  const int h = (int)(bh % (unsigned)p.heads), b = (int)(bh / (unsigned)p.heads);
  const int key0 = ks * kKS;
  if (key0 >= p.Nk) return;  // block-uniform: this slice holds no key
  const int nkeys = min(kKS, p.Nk - key0);
  const int nc = p.hd / kHD;
  const long ld = p.C, ldkv = 2L * p.C;
  const bf16_t* kb = p.kv + ((long)b * p.Nk + key0) * ldkv + h * p.hd;
  const long rowb = (long)b * p.N;
  const bf16_t* qb = p.q + rowb * ld + h * p.hd;
  const bf16_t* dob = p.d_o + rowb * ld + h * p.hd;
  const float* st = p.stats + ((long)b * p.heads + h) * p.N * 2;
  const long qbeg = (long)span * kSpanQ;

  // ---- phase 1: this wave's 32 queries against the 64 keys, contraction over the whole head dim
  {
    const long q32 = qbeg + 32 * wid;
    f32x4 s[2][4], d[2][4];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) s[qt][kt] = d[qt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (q32 < p.N) {  // wave-uniform
      for (int c = 0; c < nc; ++c) {
        u16x8 fq[2][2], fdo[2][2];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            fq[qt][kk] = gfrag(qb + c * kHD, q32 + 16 * qt + l15, p.N - 1, ld, kk, g);
            fdo[qt][kk] = gfrag(dob + c * kHD, q32 + 16 * qt + l15, p.N - 1, ld, kk, g);
          }
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            const u16x8 fk = gfrag(kb + c * kHD, 16 * kt + l15, nkeys - 1, ldkv, kk, g);
            const u16x8 fv = gfrag(kb + p.C + c * kHD, 16 * kt + l15, nkeys - 1, ldkv, kk, g);
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
              s[qt][kt] = mfma_bf16_16x16x32(fq[qt][kk], fk, s[qt][kt]);
              d[qt][kt] = mfma_bf16_16x16x32(fdo[qt][kk], fv, d[qt][kt]);
            }
          }
      }
    }
    float lse[2][4], dd[2][4];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long qi = q32 + 16 * qt + 4 * g + r;
        const bool ok = qi < p.N;
        lse[qt][r] = ok ? st[qi * 2] : INFINITY;  // exp(s - inf) = 0: a missing query contributes nothing
        dd[qt][r] = ok ? st[qi * 2 + 1] : 0.f;
      }
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const bool live = 16 * kt + l15 < nkeys;
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pv = live ? __expf(s[qt][kt][r] * p.scale - lse[qt][r]) : 0.f;
          s[qt][kt][r] = pv;
          d[qt][kt][r] = live ? p.scale * pv * (d[qt][kt][r] - dd[qt][r]) : 0.f;
        }
      sP[(wid * 4 + kt) * 64 + lane] = pack_pair(s[0][kt], s[1][kt]);
      sDS[(wid * 4 + kt) * 64 + lane] = pack_pair(d[0][kt], d[1][kt]);
    }
  }
  __syncthreads();

  // ---- phase 2: product 2c = dV chunk c (P^T dO), 2c + 1 = dK chunk c (dS^T Q); wave w takes products w, w + 4, ...
  // acc[kt][dt][r] = X[key 16 kt + 4g + r][d 16 dt + l15]: the parked fragment is the A operand, the transposed read of the
  // staged 32 x 64 tile the B operand, so one atomic instruction covers 16 consecutive floats of 4 key rows.
  const int nprod = 2 * nc > wid ? (2 * nc - wid + 3) / 4 : 0;
  const int nsteps = nprod * 4;  // four 32-query tiles per product
  bf16_t* stage = sStage + wid * 2 * 32 * kHD;
  auto issue = [&](int step) {
    const int prod = wid + 4 * (step >> 2), t = step & 3;
    const bf16_t* src = ((prod & 1) ? qb : dob) + (prod >> 1) * kHD;
    const long r0 = qbeg + 32 * t;
    char* dst = reinterpret_cast<char*>(stage + (step & 1) * 32 * kHD);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 8 * i + (lane >> 3);
      const int chunk = (lane & 7) ^ (row & 7);
      const void* sp = r0 + row < p.N ? static_cast<const void*>(src + (r0 + row) * ld + chunk * 8) : static_cast<const void*>(g_attn_zero16);
      glds16(sp, dst + i * 1024);
    }
  };
  f32x4 acc[4][4];
  if (nsteps > 0) issue(0);
  for (int step = 0; step < nsteps; ++step) {
    if (step + 1 < nsteps) {
      issue(step + 1);
      dma_wait<4>();  // the four pieces just issued may still fly; this step's tile has landed
    } else {
      dma_wait<0>();
    }
    const int prod = wid + 4 * (step >> 2), t = step & 3;
    if (t == 0) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) acc[kt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const bf16_t* tile = stage + (step & 1) * 32 * kHD;
    const u16x8* park = (prod & 1) ? sDS : sP;
    u16x8 fb[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) fb[dt] = frag_cols(tile, 4 * g, 16 + 4 * g, dt, l15);
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const u16x8 fa = park[(t * 4 + kt) * 64 + lane];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) acc[kt][dt] = mfma_bf16_16x16x32(fa, fb[dt], acc[kt][dt]);
    }
    if (t == 3) {
      float* ob = p.dkv32 + ((long)b * p.Nk + key0) * ldkv + ((prod & 1) ? 0 : p.C) + h * p.hd + (prod >> 1) * kHD;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int kl = 16 * kt + 4 * g + r;
          if (kl < nkeys) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) atomicAdd(ob + (long)kl * ldkv + 16 * dt + l15, acc[kt][dt][r]);
          }
        }
    }
  }
}

}  // namespace

// launchers behind cmda_attention_fwd / cmda_attention_bwd (attention.hip), which have checked the arguments
int attn_wide_fwd(const void* q, const void* kv, void* o, int B, int N, int Nk, int heads, int C, float scale, void* stream) {
  const int hd = C / heads;
  WideParams p{(const bf16_t*)q, (const bf16_t*)kv, nullptr, (bf16_t*)o, nullptr, nullptr, B, N, Nk, heads, C, hd, scale};
  const long nblk = (long)((N + kWideQ - 1) / kWideQ) * heads * B;
  if (nblk > 0x7fffffffL) return CMDA_ERR_SHAPE;
  dim3 grid((unsigned)nblk);
  if (Nk <= kMaxK) CMDA_LAUNCH(attn_wide_fwd_kernel<kMaxK>, grid, dim3(256), 0, stream, p);
  else CMDA_LAUNCH(attn_wide_fwd_kernel<kMaxKFwd>, grid, dim3(256), 0, stream, p);
  CMDA_CHECK_LAUNCH();
}

int attn_wide_bwd(const void* q, const void* kv, const void* d_o, void* dq, float* dkv32, float* stats, int B, int N, int Nk,
                                   int heads, int C, float scale, void* stream) {
  const int hd = C / heads;
  WideParams p{(const bf16_t*)q, (const bf16_t*)kv, (const bf16_t*)d_o, (bf16_t*)dq, dkv32, stats, B, N, Nk, heads, C, hd, scale};
  const long nb1 = (long)((N + kWideQ - 1) / kWideQ) * heads * B;
  const long nb2 = (long)((N + kSpanQ - 1) / kSpanQ) * heads * 4 * B;
  if (nb1 > 0x7fffffffL || nb2 > 0x7fffffffL) return CMDA_ERR_SHAPE;
  CMDA_LAUNCH(attn_wide_bwd_dq_kernel, dim3((unsigned)nb1), dim3(256), 0, stream, p);
  CMDA_LAUNCH(attn_wide_bwd_dkv_kernel, dim3((unsigned)nb2), dim3(256), 0, stream, p);
  CMDA_CHECK_LAUNCH();
}
