// attention.hip -- fused spatial-reduction attention core (bf16, head_dim 64, up to 256 keys): scores, softmax and the
// weighted sum of values in ONE kernel each way; the [N, Nk] score / probability matrices never reach HBM.
//
// Reference ops replaced: Attention.forward of mmseg/models/backbones/mix_transformer.py:86-103
//   attn = (q @ k.transpose(-2, -1)) * scale ; attn = attn.softmax(dim=-1) ; x = (attn @ v)      (attn_drop = 0)
// and its autograd backward.  q comes from the `q` Linear ([B*N, C], head h = columns 64h..64h+63), k / v from the `kv`
// Linear over the spatially reduced tokens ([B*Nk, 2C]: K at column 64h, V at column C + 64h).  With CMDA's 512x512
// crops every stage has Nk = 256 keys (sr_ratios 8/4/2/1), which is what makes the whole key set fit in LDS.
//
// Orientation: everything is computed TRANSPOSED, S^T = K Q^T, so that the MFMA result layout (row = 4*(lane>>4)+r,
// col = lane&15) puts the keys on (lane>>4, r) and the queries on lane&15.  Then
//   * the softmax over keys is a per-lane reduction plus two xor-shuffles (16, 32),
//   * P^T is already in the B-operand layout of the second GEMM O^T = V^T P^T (k = keys): no LDS round trip for P,
//   * V^T is read from the row-major V tile with ds_read_b64_tr_b16.
// The k index of an MFMA is a free labelling as long as A and B agree; here slot (g, j) of the u-th group of 32 keys is
// key 32u + 4g + j (j < 4) or 32u + 16 + 4g + (j - 4), i.e. exactly the accumulator registers of score tiles 2u and 2u+1.
//
// MFMA-bound per block but small: per 16 queries 32 + 32 v_mfma_f32_16x16x32_bf16.  HBM traffic per (batch, head):
// Q, O once, K, V once per 128-query block (L2 hits).  Algorithmic bytes per query: 2 * 64 * 2 (q, o) + the K/V share.
//
// Precision policy: the kernels are written once and instantiated for AttnBf16 and AttnSplit (cmda dtype CMDA_F32X3: fp32 storage,
// every product as three bf16 MFMAs a_lo b_hi + a_hi b_lo + a_hi b_hi with fp32 accumulation, ~16 mantissa bits per product -- the
// arithmetic of gemm_x3_lean.hip).  A policy fixes the storage type of q / o / dO / dq / direct dK | dV, the number P of bf16 images an
// operand has (Frag<Prec>: P register sets; K and V: P LDS tiles each, 4 x 32 KB and one workgroup per CU when split) and the launch
// constants; everything else is the same text.  Split operands are split ONCE: K and V in
// HBM by the caller, the query-side fragments in registers, the probabilities and dS in registers right where the bf16 form packs them.
// Two instances measured slower than the kernels they replace and stay kernels of their own, next to the templates: the masked bf16 dQ
// kernel (attn_bwd_dq_masked_kernel) and the split-bf16 dK | dV kernel (attn_bwd_dkv_x3_kernel); the reasons are at their definitions.
// (Before the split-bf16 instances that mode's attention ran as batched Q K^T / softmax / P V GEMMs + four backward products + two
// softmax launches with the [N, Nk] probabilities in HBM, mix_transformer.py:97-101; ~20 ms of that mode's kernel time per UDA step.
// Their first version converted K / V per block in registers, which cost as much as the block's MFMAs: 116.4 against 116.8 ms per step;
// with kv split once in HBM 113.3 ms.)
#include "attention_common.h"

namespace {

struct AttnBf16 {
  using Elem = bf16_t;
  static constexpr int P = 1;
  static constexpr int kBlocksPerCU = 2;  // of the four-wave kernels (2 x 32 KB of K / V)
  // queries per block of the forward-shaped kernels: 64 (one pass of 4 waves x 16) or 128 (two passes, K/V loaded once for
  // both) -- the launcher takes 64 while that still leaves the grid under ~4 blocks per CU (stage 3: 27.4 -> 22.9 us).
  // The full-key instances' passes are half as long, so the K / V fill weighs more: they take 128 from 512 blocks of 128 up, the grid
  // that fills the 512 block slots of the chip once (graph-timed forward, 64 | 128 per block: 512 blocks of 128 11.6 | 9.9 and
  // 10.5 | 9.2 us, 320 blocks 9.5 | 8.8, 256 blocks 6.5 | 7.4 and 6.1 | 7.0; profiles/attn_fullkeys_bench.txt)
  static constexpr long block_switch(bool full) { return full ? 512 : 1024; }
  static constexpr long kSpanTarget = 512;  // dK | dV blocks to reach with query spans: ~2 per CU
};

struct AttnSplit {
  using Elem = float;
  static constexpr int P = 2;  // images (hi, lo): hi = bf16(x), lo = bf16(x - hi)
  static constexpr int kBlocksPerCU = 1;
  // one workgroup per CU (128 KB of K / V images): 64 queries while the grid is under two rounds
  static constexpr long block_switch(bool) { return 256; }
  static constexpr long kSpanTarget = 256;
};

template <class Prec>
static inline int fwd_queries_per_block(int B, int N, int heads, bool full) {
  return (long)((N + 127) / 128) * heads * B < Prec::block_switch(full) ? 64 : 128;
}

// one MFMA operand: P bf16 images of 8 values
template <class Prec>
struct Frag {
  u16x8 v[Prec::P];
};

static __device__ __forceinline__ f32x4 mma(const Frag<AttnBf16>& a, const Frag<AttnBf16>& b, f32x4 c) {
  return mfma_bf16_16x16x32(a.v[0], b.v[0], c);
}
// c += a b with a = (a_hi, a_lo), b = (b_hi, b_lo): the three significant partial products
static __device__ __forceinline__ f32x4 mma(const Frag<AttnSplit>& a, const Frag<AttnSplit>& b, f32x4 c) {
  c = mfma_bf16_16x16x32(a.v[1], b.v[0], c);
  c = mfma_bf16_16x16x32(a.v[0], b.v[1], c);
  return mfma_bf16_16x16x32(a.v[0], b.v[0], c);
}

// frag_rows / frag_cols of every image of a [P][rows * 64] LDS tile
template <class Prec, int L>
static __device__ __forceinline__ Frag<Prec> frag_rows(const bf16_t (*tile)[L], int row0, int kk, int g, int l15) {
  Frag<Prec> f;
#pragma unroll
  for (int i = 0; i < Prec::P; ++i) f.v[i] = frag_rows(tile[i], row0, kk, g, l15);
  return f;
}
template <class Prec, int L>
static __device__ __forceinline__ Frag<Prec> frag_cols(const bf16_t (*tile)[L], int R0, int R1, int dt, int l15) {
  Frag<Prec> f;
#pragma unroll
  for (int i = 0; i < Prec::P; ++i) f.v[i] = frag_cols(tile[i], R0, R1, dt, l15);
  return f;
}

static __device__ __forceinline__ void split4(const float (&x)[4], u16x4& hi, u16x4& lo) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bf16_t h = f2bf(x[e]);
    hi[e] = h;
    lo[e] = f2bf(x[e] - bf2f(h));
  }
}

template <class Prec>
static __device__ __forceinline__ Frag<Prec> pack_pair(const f32x4& a, const f32x4& b) {
  Frag<Prec> f;
  if constexpr (Prec::P == 1) {
    f.v[0] = pack_pair(a, b);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bf16_t ha = f2bf(a[r]), hb = f2bf(b[r]);
      f.v[0][r] = ha; f.v[0][4 + r] = hb;
      f.v[1][r] = f2bf(a[r] - bf2f(ha)); f.v[1][4 + r] = f2bf(b[r] - bf2f(hb));
    }
  }
  return f;
}

// B operand b[k = d][col = query] of 16 consecutive rows of a [rows, ld] global matrix (rows past `nrows` repeat the last):
// lane (l15, g) reads d = 32 kk + 8 g .. + 7 -- load_qfrag of attention_common.h, and its fp32 form split in registers
static __device__ __forceinline__ void load_qfrag(const bf16_t* __restrict__ base, long row0, long nrows, int ld, int g, int l15,
                                                  Frag<AttnBf16> (&f)[2]) {
  u16x8 t[2];
  load_qfrag(base, row0, nrows, ld, g, l15, t);
  f[0].v[0] = t[0];
  f[1].v[0] = t[1];
}
static __device__ __forceinline__ void load_qfrag(const float* __restrict__ base, long row0, long nrows, int ld, int g, int l15,
                                                  Frag<AttnSplit> (&f)[2]) {
  long row = row0 + l15;
  if (row >= nrows) row = nrows - 1;
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    float a[4], b[4];
    ld4(base + row * ld + 32 * kk + 8 * g, a);
    ld4(base + row * ld + 32 * kk + 8 * g + 4, b);
    u16x4 ah, al, bh, bl;
    split4(a, ah, al);
    split4(b, bh, bl);
    f[kk].v[0] = u16x8{ah[0], ah[1], ah[2], ah[3], bh[0], bh[1], bh[2], bh[3]};
    f[kk].v[1] = u16x8{al[0], al[1], al[2], al[3], bl[0], bl[1], bl[2], bl[3]};
  }
}

// raw scores^T of 16 queries against the key tiles: p[t][r] = S^T[key 16t + 4g + r][query l15], unscaled; softmax_keys or
// exp_keys_full turns them into probabilities
template <class Prec, int NT, bool FULL, int L>
static __device__ __forceinline__ void raw_scores(const bf16_t (*sK)[L], const Frag<Prec> (&qf)[2], int nt, int g, int l15, f32x4 (&p)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    p[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (FULL || t < nt) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) p[t] = mma(frag_rows<Prec>(sK, 16 * t, kk, g, l15), qf[kk], p[t]);
    }
  }
}

// K | V of MAXK key rows of one (batch, head) -> the P images of sK and sV
template <class Prec, int MAXK>
static __device__ __forceinline__ void load_kv_images(const bf16_t* const (&kv)[Prec::P], long off, int C, int Nk, bf16_t (*sK)[MAXK * kHD],
                                                      bf16_t (*sV)[MAXK * kHD], int wid, int lane) {
#pragma unroll
  for (int i = 0; i < Prec::P; ++i) load_kv_tile<MAXK>(kv[i] + off, 2 * C, Nk, sK[i], wid, lane, 4);
#pragma unroll
  for (int i = 0; i < Prec::P; ++i) load_kv_tile<MAXK>(kv[i] + off + C, 2 * C, Nk, sV[i], wid, lane, 4);
}

template <class Prec>
struct AttnParams {
  const typename Prec::Elem* q;  // [B*N, C]
  // [B*Nk, 2C]; split-bf16: kv split ONCE in HBM by the caller (cmda_split_bf16) -- every query block of a (batch, head) reads the same K / V
  const bf16_t* kv[Prec::P];
  typename Prec::Elem* o;        // [B*N, C]
  int B, N, Nk, heads, C;
  float scale;
  int q_per_block;
};

// MAXK: keys held in LDS -- 256 (every stage of a 512 x 512 crop; two blocks per CU) or 320 (inference on 440 x 640 frames,
// encoder_decoder.py:897-936: 260 / 280 keys after the spatial reduction; forward only, one block per CU).
// FULL: Nk == MAXK and scale > 0 (every training launch: 256 keys at every stage) -- the full-key form of attention_common.h: no key
// mask (64 compares + selects per lane and the SGPR spills of their lane masks), no tile guards, unnormalised probabilities into the
// second GEMM and 1 / l applied to the 16 outputs.  The masked form serves every other key count and is the reference for it.
template <class Prec, int MAXK, bool FULL = false>
__global__ __launch_bounds__(256, MAXK <= 256 ? Prec::kBlocksPerCU : 1) void attn_fwd_kernel(AttnParams<Prec> p) {
  constexpr int NT = MAXK / 16;
  const int Nk = FULL ? MAXK : p.Nk;
  __shared__ __attribute__((aligned(1024))) bf16_t sK[Prec::P][MAXK * kHD];
  __shared__ __attribute__((aligned(1024))) bf16_t sV[Prec::P][MAXK * kHD];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, l15 = lane & 15;
  const unsigned nqb = (unsigned)((p.N + p.q_per_block - 1) / p.q_per_block);
  const unsigned lb = xcd_logical_block(), bh = lb / nqb;
  const long qblk = lb - bh * nqb;
  const int h = (int)(bh % (unsigned)p.heads), b = (int)(bh / (unsigned)p.heads);
  load_kv_images<Prec, MAXK>(p.kv, (long)b * Nk * 2 * p.C + h * kHD, p.C, Nk, sK, sV, wid, lane);
  __syncthreads();
  const int nt = (Nk + 15) >> 4;
  const typename Prec::Elem* qb = p.q + (long)b * p.N * p.C + h * kHD;
  typename Prec::Elem* ob = p.o + (long)b * p.N * p.C + h * kHD;
  for (int pass = 0; pass < p.q_per_block / 64; ++pass) {
    const long q0 = qblk * p.q_per_block + pass * 64 + wid * 16;
    if (q0 >= p.N) break;  // wave-uniform
    Frag<Prec> qf[2];
    load_qfrag(qb, q0, p.N, p.C, g, l15, qf);
    f32x4 pr[NT];
    float inv = 1.f;
    raw_scores<Prec, NT, FULL>(sK, qf, nt, g, l15, pr);
    if constexpr (FULL) inv = exp_keys_full<NT>(p.scale, pr);
    else softmax_keys<NT>(Nk, p.scale, g, pr);
    f32x4 oacc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < NT / 2; ++u) {
      if (FULL || 2 * u < nt) {
        const Frag<Prec> pb = pack_pair<Prec>(pr[2 * u], pr[2 * u + 1]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          oacc[dt] = mma(frag_cols<Prec>(sV, 32 * u + 4 * g, 32 * u + 16 + 4 * g, dt, l15), pb, oacc[dt]);
      }
    }
    if (q0 + l15 < p.N) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        if constexpr (FULL) oacc[dt] *= inv;
        const float v[4] = {oacc[dt][0], oacc[dt][1], oacc[dt][2], oacc[dt][3]};
        st4(ob + (q0 + l15) * p.C + 16 * dt + 4 * g, v);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Backward = two kernels, both recomputing the probabilities from q / k (nothing but q, kv, o-gradient is read):
//   attn_bwd_dq_kernel   (forward-shaped: 16 queries per wave, all keys in LDS)
//       P^T = softmax(K Q^T), dP^T = V dO^T, D = sum_k P dP, dS^T = scale * P (dP - D), dQ^T = K^T dS^T -> dq
//       and per query the softmax log-sum-exp and D -> stats[b, h, q, 2] for the second kernel
//   attn_bwd_dkv_kernel  (block = one 64-key slice of one (batch, head) x a span of queries; wave = 32 queries at a time)
//       S = Q K^T for the slice, P = exp(scale*S - lse), dP = dO V^T, dS = scale * P (dP - D)       [query][key] tiles
//       dV^T += dO^T P,  dK^T += Q^T dS      (contraction over the 32 queries; P / dS are B operands straight from the
//       accumulator registers, dO^T / Q^T are transposed LDS reads of the wave's staged 32 x 64 tiles)
//       waves fold their partial dK^T / dV^T through LDS, then one fp32 atomic per element per block.
// (The first version did all of it in one kernel with P / dS staged in LDS: 144 KiB of LDS and 512 registers meant one
// wave per SIMD and ~21 us per 64-query chunk -- latency-bound.  Split this way the kernels run 8 / 12 waves per CU.)
template <class Prec>
struct AttnBwdParams {
  const typename Prec::Elem* q;
  const bf16_t* kv[Prec::P];
  const typename Prec::Elem* d_o;
  typename Prec::Elem* dq;
  float* dkv32;                     // accumulate mode: fp32 atomics (zero on entry)
  typename Prec::Elem* dkv_direct;  // direct mode (one query span per key slice): dK | dV stored, no atomics, no workspace
  float* stats;  // [B, heads, N, 2] = (lse, D)
  int B, N, Nk, heads, C, q_per_block;
  float scale;
  int fwd_q_per_block;  // of the dQ kernel
  int spans;            // query spans of the dK/dV kernel
};

// FULL: Nk == kMaxK and scale > 0, the full-key form (attn_fwd_kernel).  With e = l P the unnormalised exponentials and inv = 1 / l:
//   D = inv * sum_k e dP,   dS^T = (scale inv) e (dP - D),   and since dQ^T = K^T dS^T is linear in dS the factor scale * inv is applied
//   to the 16 dQ accumulators, not to the 64 dS values: what is packed for the last GEMM is e (dP - D).
// stats[b, h, q, 2] = (lse of the scaled scores, D) is the same contract with attn_bwd_dkv_kernel in both forms.
template <class Prec, bool FULL = false>
__global__ __launch_bounds__(256, Prec::kBlocksPerCU) void attn_bwd_dq_kernel(AttnBwdParams<Prec> p) {
  using Elem = typename Prec::Elem;
  __shared__ __attribute__((aligned(1024))) bf16_t sK[Prec::P][kMaxK * kHD];
  __shared__ __attribute__((aligned(1024))) bf16_t sV[Prec::P][kMaxK * kHD];
  const int Nk = FULL ? kMaxK : p.Nk;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, l15 = lane & 15;
  const unsigned nqb = (unsigned)((p.N + p.fwd_q_per_block - 1) / p.fwd_q_per_block);
  const unsigned lb = xcd_logical_block(), bh = lb / nqb;
  const long qblk = lb - bh * nqb;
  const int h = (int)(bh % (unsigned)p.heads), b = (int)(bh / (unsigned)p.heads);
  load_kv_images<Prec, kMaxK>(p.kv, (long)b * Nk * 2 * p.C + h * kHD, p.C, Nk, sK, sV, wid, lane);
  __syncthreads();
  const int nt = (Nk + 15) >> 4;
  const long rowb = (long)b * p.N;
  const Elem* qb = p.q + rowb * p.C + h * kHD;
  const Elem* dob = p.d_o + rowb * p.C + h * kHD;
  Elem* dqb = p.dq + rowb * p.C + h * kHD;
  float* st = p.stats + ((long)b * p.heads + h) * p.N * 2;
  for (int pass = 0; pass < p.fwd_q_per_block / 64; ++pass) {
    const long q0 = qblk * p.fwd_q_per_block + pass * 64 + wid * 16;
    if (q0 >= p.N) break;  // wave-uniform
    Frag<Prec> qf[2], dof[2];
    load_qfrag(qb, q0, p.N, p.C, g, l15, qf);
    load_qfrag(dob, q0, p.N, p.C, g, l15, dof);
    f32x4 pr[kNT], dp[kNT];
    float lse, inv = 1.f;
    raw_scores<Prec, kNT, FULL>(sK, qf, nt, g, l15, pr);
    if constexpr (FULL) inv = exp_keys_full(p.scale, pr, &lse);
    else softmax_keys(Nk, p.scale, g, pr, &lse);
    float dsum = 0.f;
#pragma unroll
    for (int t = 0; t < kNT; ++t) {
      dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (FULL || t < nt) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) dp[t] = mma(frag_rows<Prec>(sV, 16 * t, kk, g, l15), dof[kk], dp[t]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) dsum += pr[t][r] * dp[t][r];
    }
    dsum = col_sum(dsum);
    if constexpr (FULL) dsum *= inv;
#pragma unroll
    for (int t = 0; t < kNT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if constexpr (FULL) dp[t][r] = pr[t][r] * (dp[t][r] - dsum);  // dS^T / (scale inv)
        else dp[t][r] = p.scale * pr[t][r] * (dp[t][r] - dsum);       // dS^T
      }
    f32x4 dqacc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dqacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < kNT / 2; ++u) {
      if (FULL || 2 * u < nt) {
        const Frag<Prec> db = pack_pair<Prec>(dp[2 * u], dp[2 * u + 1]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          dqacc[dt] = mma(frag_cols<Prec>(sK, 32 * u + 4 * g, 32 * u + 16 + 4 * g, dt, l15), db, dqacc[dt]);
      }
    }
    if (q0 + l15 < p.N) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        if constexpr (FULL) dqacc[dt] *= p.scale * inv;
        const float v[4] = {dqacc[dt][0], dqacc[dt][1], dqacc[dt][2], dqacc[dt][3]};
        st4(dqb + (q0 + l15) * p.C + 16 * dt + 4 * g, v);
      }
      if (g == 0) {
        st[(q0 + l15) * 2 + 0] = lse;
        st[(q0 + l15) * 2 + 1] = dsum;
      }
    }
  }
}

// The masked bf16 dQ kernel is kept as the parent's own kernel, not the instance <AttnBf16, false> of attn_bwd_dq_kernel: as an instance the
// compiler folds the four dQ accumulators into one 16-float value across the tile guards (246 -> 256 VGPRs, +10 VALU, +39 SALU instructions)
// and the backward at 255 keys measured 0.2 us slower at three of the stage shapes (profiles/attn_one_source_bench.txt).  The scores have to
// come through a helper of their own for that: with the same loop written in the kernel body this copy compiles to the 256 registers too.
template <int NT = kNT>
static __device__ __forceinline__ void scores_softmax(const bf16_t* sK, const u16x8 (&qf)[2], int nt, int Nk, float scale,
                                                      int g, int l15, f32x4 (&p)[NT], float* lse_out = nullptr) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    p[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (t < nt) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) p[t] = mfma_bf16_16x16x32(frag_rows(sK, 16 * t, kk, g, l15), qf[kk], p[t]);
    }
  }
  softmax_keys<NT>(Nk, scale, g, p, lse_out);
}

__global__ __launch_bounds__(256, 2) void attn_bwd_dq_masked_kernel(AttnBwdParams<AttnBf16> p) {
  __shared__ __attribute__((aligned(1024))) bf16_t sK[kMaxK * kHD];
  __shared__ __attribute__((aligned(1024))) bf16_t sV[kMaxK * kHD];
  const int Nk = p.Nk;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, l15 = lane & 15;
  const unsigned nqb = (unsigned)((p.N + p.fwd_q_per_block - 1) / p.fwd_q_per_block);
  const unsigned lb = xcd_logical_block(), bh = lb / nqb;
  const long qblk = lb - bh * nqb;
  const int h = (int)(bh % (unsigned)p.heads), b = (int)(bh / (unsigned)p.heads);
  const bf16_t* kbase = p.kv[0] + (long)b * Nk * 2 * p.C + h * kHD;
  load_kv_tile(kbase, 2 * p.C, Nk, sK, wid, lane, 4);
  load_kv_tile(kbase + p.C, 2 * p.C, Nk, sV, wid, lane, 4);
  __syncthreads();
  const int nt = (Nk + 15) >> 4;
  const long rowb = (long)b * p.N;
  const bf16_t* qb = p.q + rowb * p.C + h * kHD;
  const bf16_t* dob = p.d_o + rowb * p.C + h * kHD;
  bf16_t* dqb = p.dq + rowb * p.C + h * kHD;
  float* st = p.stats + ((long)b * p.heads + h) * p.N * 2;
  for (int pass = 0; pass < p.fwd_q_per_block / 64; ++pass) {
    const long q0 = qblk * p.fwd_q_per_block + pass * 64 + wid * 16;
    if (q0 >= p.N) break;  // wave-uniform
    u16x8 qf[2], dof[2];
    load_qfrag(qb, q0, p.N, p.C, g, l15, qf);
    load_qfrag(dob, q0, p.N, p.C, g, l15, dof);
    f32x4 pr[kNT], dp[kNT];
    float lse;
    scores_softmax(sK, qf, nt, Nk, p.scale, g, l15, pr, &lse);
    float dsum = 0.f;
#pragma unroll
    for (int t = 0; t < kNT; ++t) {
      dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t < nt) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) dp[t] = mfma_bf16_16x16x32(frag_rows(sV, 16 * t, kk, g, l15), dof[kk], dp[t]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) dsum += pr[t][r] * dp[t][r];
    }
    dsum = col_sum(dsum);
#pragma unroll
    for (int t = 0; t < kNT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) dp[t][r] = p.scale * pr[t][r] * (dp[t][r] - dsum);  // dS^T
    f32x4 dqacc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dqacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < kNT / 2; ++u) {
      if (2 * u < nt) {
        const u16x8 db = pack_pair(dp[2 * u], dp[2 * u + 1]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          dqacc[dt] = mfma_bf16_16x16x32(frag_cols(sK, 32 * u + 4 * g, 32 * u + 16 + 4 * g, dt, l15), db, dqacc[dt]);
      }
    }
    if (q0 + l15 < p.N) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const float v[4] = {dqacc[dt][0], dqacc[dt][1], dqacc[dt][2], dqacc[dt][3]};
        st4(dqb + (q0 + l15) * p.C + 16 * dt + 4 * g, v);
      }
      if (g == 0) {
        st[(q0 + l15) * 2 + 0] = lse;
        st[(q0 + l15) * 2 + 1] = dsum;
      }
    }
  }
}

constexpr int kRedPitch = 68;  // floats per key row of the cross-wave reduction buffer

// ---- the dK | dV kernel's staging of one wave's 32 rows of Q and dO (rows past N read as zero) into its P-image tiles sQ, sDO,
// and the wait that makes the tiles readable.  bf16: LDS DMA, issued before the caller's lse / D loads and waited for after them.
static __device__ __forceinline__ void stage_q_do(const bf16_t* qb, const bf16_t* dob, long q32, int N, int C, bf16_t (*sQ)[32 * kHD],
                                                  bf16_t (*sDO)[32 * kHD], int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = 8 * i + (lane >> 3);
    const int chunk = (lane & 7) ^ (row & 7);
    const bool ok = q32 + row < N;
    const void* zero = static_cast<const void*>(g_attn_zero16);
    glds16(ok ? static_cast<const void*>(qb + (q32 + row) * C + chunk * 8) : zero, reinterpret_cast<char*>(sQ[0]) + i * 1024);
    glds16(ok ? static_cast<const void*>(dob + (q32 + row) * C + chunk * 8) : zero, reinterpret_cast<char*>(sDO[0]) + i * 1024);
  }
}
static __device__ __forceinline__ void stage_wait(AttnBf16) { dma_wait<0>(); }

// this wave's LDS stores are visible to its own later LDS reads (cross-lane hand-off inside ONE wave: DS operations of a wave execute in
// order; the statement also keeps the compiler from moving the reads up)
#ifndef CMDA_EMU
static __device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
#else
static inline void wave_lds_sync() { emu::wave_barrier(); }
#endif

// rows [0, rows) of an fp32 [*, ld] matrix (64 columns at src) -> hi / lo images [rows][64] bf16 in the swizzled layout of load_kv_tile
// (16-byte chunk c of line r at slot c ^ (r & 7)); rows >= nvalid are zero.  Thread t of nthr converts one float4 per step.
static __device__ __forceinline__ void load_split_tile(const float* __restrict__ src, long ld, int nvalid, int rows, bf16_t* hi, bf16_t* lo,
                                                       int t, int nthr) {
  for (int i = t; i < rows * 16; i += nthr) {
    const int row = i >> 4, c4 = i & 15;
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    if (row < nvalid) ld4(src + (long)row * ld + 4 * c4, x);
    u16x4 h, l;
    split4(x, h, l);
    const int off = row * kHD + ((((c4 >> 1) ^ (row & 7))) << 3) + ((c4 & 1) << 2);
    *reinterpret_cast<u16x4*>(hi + off) = h;
    *reinterpret_cast<u16x4*>(lo + off) = l;
  }
}


// NW waves per block: 4 (two blocks per CU when the queries are split into spans) or 8 (direct mode: one block per key slice walks
// every query, 80 ... 160 blocks per launch -- the walk is a serial chain of DMA -> MFMA steps per wave, so twice the waves halve it)
template <class Prec, int NW>
__global__ __launch_bounds__(64 * NW, NW == 4 ? Prec::kBlocksPerCU : 1) void attn_bwd_dkv_kernel(AttnBwdParams<Prec> p) {
  using Elem = typename Prec::Elem;
  constexpr int P = Prec::P;
  __shared__ __attribute__((aligned(1024))) bf16_t sK[P][kKS * kHD];
  __shared__ __attribute__((aligned(1024))) bf16_t sV[P][kKS * kHD];
  constexpr int kStageBytes = NW * 2 * P * 32 * kHD * 2;      // per wave: the P images of the Q and dO tiles of 32 queries
  constexpr int kRedBytes = 2 * kKS * kRedPitch * 4;          // dK | dV as [key][d] fp32
  __shared__ __attribute__((aligned(1024))) char sbuf[kStageBytes > kRedBytes ? kStageBytes : kRedBytes];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, l15 = lane & 15;
  // logical order: key slice fastest (the four slices of one (batch, head, span) stream the same Q / dO rows), then span
  const unsigned lb = xcd_logical_block();
  const int ks = (int)(lb & 3);
  const unsigned span = (lb >> 2) % (unsigned)p.spans, bh = (lb >> 2) / (unsigned)p.spans;
  const int h = (int)(bh % (unsigned)p.heads), b = (int)(bh / (unsigned)p.heads);
  const int key0 = ks * kKS;
  if (key0 >= p.Nk) return;  // block-uniform: this slice holds no key
  const int nkeys = min(kKS, p.Nk - key0);
  // p.kv is read with constant indices: indexed by a loop variable the kernel-argument loads stay where the loop is unrolled, and the
  // different schedule costs the bf16 instances registers (dkv<8>: 16 spills against 15; 0.3-0.6 us per launch at the span shapes)
  const long koff = ((long)b * p.Nk + key0) * 2 * p.C + h * kHD;
  const bf16_t* kbase[P] = {p.kv[0] + koff};
  if constexpr (P == 2) kbase[1] = p.kv[1] + koff;
  for (int i = wid; i < kKS / 8; i += NW) {
    const int row = 8 * i + (lane >> 3);
    const int chunk = (lane & 7) ^ (row & 7);
    const void* zero = static_cast<const void*>(g_attn_zero16);
    const bool ok = row < nkeys;
#pragma unroll
    for (int j = 0; j < P; ++j)
      glds16(ok ? static_cast<const void*>(kbase[j] + (long)row * 2 * p.C + chunk * 8) : zero, reinterpret_cast<char*>(sK[j]) + i * 1024);
#pragma unroll
    for (int j = 0; j < P; ++j)
      glds16(ok ? static_cast<const void*>(kbase[j] + (long)row * 2 * p.C + chunk * 8 + p.C) : zero, reinterpret_cast<char*>(sV[j]) + i * 1024);
  }
  __syncthreads();
  const long rowb = (long)b * p.N;
  const Elem* qb = p.q + rowb * p.C + h * kHD;
  const Elem* dob = p.d_o + rowb * p.C + h * kHD;
  const float* st = p.stats + ((long)b * p.heads + h) * p.N * 2;
  using Tile = bf16_t[32 * kHD];
  Tile* sQw = reinterpret_cast<Tile*>(reinterpret_cast<bf16_t*>(sbuf) + wid * 2 * P * 32 * kHD);  // this wave's Q images, then its dO images
  Tile* sDOw = sQw + P;

  f32x4 dvacc[4][4], dkacc[4][4];  // [d tile][key tile]: dV^T, dK^T
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) dvacc[dt][kt] = dkacc[dt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const long qbeg = (long)span * p.q_per_block;
  const long qend = min((long)p.N, qbeg + p.q_per_block);
  for (long q32 = qbeg + 32 * wid; q32 < qend; q32 += 32 * NW) {
    stage_q_do(qb, dob, q32, p.N, p.C, sQw, sDOw, lane);
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
    stage_wait(Prec{});
    f32x4 pr[2][4], ds[2][4];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      Frag<Prec> fq[2], fdo[2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        fq[kk] = frag_rows<Prec>(sQw, 16 * qt, kk, g, l15);
        fdo[kk] = frag_rows<Prec>(sDOw, 16 * qt, kk, g, l15);
      }
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, d = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          s = mma(fq[kk], frag_rows<Prec>(sK, 16 * kt, kk, g, l15), s);
          d = mma(fdo[kk], frag_rows<Prec>(sV, 16 * kt, kk, g, l15), d);
        }
        const bool live = 16 * kt + l15 < nkeys;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pv = live ? __expf(s[r] * p.scale - lse[qt][r]) : 0.f;
          pr[qt][kt][r] = pv;
          ds[qt][kt][r] = p.scale * pv * (d[r] - dd[qt][r]);
        }
      }
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const Frag<Prec> fdoT = frag_cols<Prec>(sDOw, 4 * g, 16 + 4 * g, dt, l15);
      const Frag<Prec> fqT = frag_cols<Prec>(sQw, 4 * g, 16 + 4 * g, dt, l15);
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        dvacc[dt][kt] = mma(fdoT, pack_pair<Prec>(pr[0][kt], pr[1][kt]), dvacc[dt][kt]);
        dkacc[dt][kt] = mma(fqT, pack_pair<Prec>(ds[0][kt], ds[1][kt]), dkacc[dt][kt]);
      }
    }
  }
  // ---- fold the waves' partials through LDS ([key][d], pitch 68), then store (direct mode) or one atomic per element
  __syncthreads();  // every wave is done with its staging tiles (the buffer is reused)
  float* red = reinterpret_cast<float*>(sbuf);
  for (int w = 0; w < NW; ++w) {
    if (wid == w) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          float* rk = red + (16 * kt + l15) * kRedPitch + 16 * dt + 4 * g;
          float* rv = rk + kKS * kRedPitch;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            rk[r] = (w ? rk[r] : 0.f) + dkacc[dt][kt][r];
            rv[r] = (w ? rv[r] : 0.f) + dvacc[dt][kt][r];
          }
        }
    }
    __syncthreads();
  }
  if (p.dkv_direct) {  // this block saw every query of its (batch, head, key slice): the sums are final
    Elem* ob = p.dkv_direct + ((long)b * p.Nk + key0) * 2 * p.C + h * kHD;
    for (int e = tid; e < kKS * kHD; e += 64 * NW) {
      const int kl = e >> 6, d = e & 63;
      if (kl < nkeys) {
        stf(ob + (long)kl * 2 * p.C + d, red[kl * kRedPitch + d]);
        stf(ob + (long)kl * 2 * p.C + p.C + d, red[(kKS + kl) * kRedPitch + d]);
      }
    }
    return;
  }
  float* ob = p.dkv32 + ((long)b * p.Nk + key0) * 2 * p.C + h * kHD;
  for (int e = tid; e < kKS * kHD; e += 64 * NW) {
    const int kl = e >> 6, d = e & 63;
    if (kl < nkeys) {
      atomicAdd(ob + (long)kl * 2 * p.C + d, red[kl * kRedPitch + d]);
      atomicAdd(ob + (long)kl * 2 * p.C + p.C + d, red[(kKS + kl) * kRedPitch + d]);
    }
  }
}

// dK | dV, split-bf16: four waves per 64-key slice; per wave the 32 x 64 tiles of Q and dO as hi / lo images (4 x 4 KB).
// Kept as its own kernel, not an instance of attn_bwd_dkv_kernel: as an instance (same query loop, opcode for opcode) its direct-mode launch
// of 40 blocks measured ~0.5 us of 56 slower (profiles/attn_one_source_bench.txt).
static __device__ __forceinline__ f32x4 mfma_x3(u16x8 ah, u16x8 al, u16x8 bh, u16x8 bl, f32x4 c) {
  return mma(Frag<AttnSplit>{{ah, al}}, Frag<AttnSplit>{{bh, bl}}, c);
}
static __device__ __forceinline__ void pack_pair_x3(const f32x4& a, const f32x4& b, u16x8& hi, u16x8& lo) {
  const Frag<AttnSplit> f = pack_pair<AttnSplit>(a, b);
  hi = f.v[0];
  lo = f.v[1];
}
__global__ __launch_bounds__(256, 1) void attn_bwd_dkv_x3_kernel(AttnBwdParams<AttnSplit> p) {
  constexpr int NW = 4;
  __shared__ __attribute__((aligned(1024))) bf16_t sKh[kKS * kHD];
  __shared__ __attribute__((aligned(1024))) bf16_t sKl[kKS * kHD];
  __shared__ __attribute__((aligned(1024))) bf16_t sVh[kKS * kHD];
  __shared__ __attribute__((aligned(1024))) bf16_t sVl[kKS * kHD];
  constexpr int kStageBytes = NW * 4 * 32 * kHD * 2;          // per wave: Q hi / lo and dO hi / lo tiles of 32 queries
  constexpr int kRedBytes = 2 * kKS * kRedPitch * 4;          // dK | dV as [key][d] fp32
  __shared__ __attribute__((aligned(1024))) char sbuf[kStageBytes > kRedBytes ? kStageBytes : kRedBytes];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, l15 = lane & 15;
  const unsigned lb = xcd_logical_block();
  const int ks = (int)(lb & 3);
  const unsigned span = (lb >> 2) % (unsigned)p.spans, bh = (lb >> 2) / (unsigned)p.spans;
  const int h = (int)(bh % (unsigned)p.heads), b = (int)(bh / (unsigned)p.heads);
  const int key0 = ks * kKS;
  if (key0 >= p.Nk) return;  // block-uniform: this slice holds no key
  const int nkeys = min(kKS, p.Nk - key0);
  const long koff = ((long)b * p.Nk + key0) * 2 * p.C + h * kHD;
  for (int i = wid; i < kKS / 8; i += NW) {
    const int row = 8 * i + (lane >> 3);
    const int chunk = (lane & 7) ^ (row & 7);
    const void* zero = static_cast<const void*>(g_attn_zero16);
    const long so = koff + (long)row * 2 * p.C + chunk * 8;
    const bool ok = row < nkeys;
    glds16(ok ? static_cast<const void*>(p.kv[0] + so) : zero, reinterpret_cast<char*>(sKh) + i * 1024);
    glds16(ok ? static_cast<const void*>(p.kv[1] + so) : zero, reinterpret_cast<char*>(sKl) + i * 1024);
    glds16(ok ? static_cast<const void*>(p.kv[0] + so + p.C) : zero, reinterpret_cast<char*>(sVh) + i * 1024);
    glds16(ok ? static_cast<const void*>(p.kv[1] + so + p.C) : zero, reinterpret_cast<char*>(sVl) + i * 1024);
  }
  __syncthreads();
  const long rowb = (long)b * p.N;
  const float* qb = p.q + rowb * p.C + h * kHD;
  const float* dob = p.d_o + rowb * p.C + h * kHD;
  const float* st = p.stats + ((long)b * p.heads + h) * p.N * 2;
  bf16_t* sQh = reinterpret_cast<bf16_t*>(sbuf) + wid * 4 * 32 * kHD;
  bf16_t* sQl = sQh + 32 * kHD;
  bf16_t* sDh = sQl + 32 * kHD;
  bf16_t* sDl = sDh + 32 * kHD;

  f32x4 dvacc[4][4], dkacc[4][4];  // [d tile][key tile]: dV^T, dK^T
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) dvacc[dt][kt] = dkacc[dt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const long qbeg = (long)span * p.q_per_block;
  const long qend = min((long)p.N, qbeg + p.q_per_block);
  for (long q32 = qbeg + 32 * wid; q32 < qend; q32 += 32 * NW) {
    wave_lds_sync();   // the previous trip's fragment reads are done before the tiles are overwritten
    const int nq = (int)min(32L, p.N - q32);
    load_split_tile(qb + q32 * p.C, p.C, nq, 32, sQh, sQl, lane, 64);
    load_split_tile(dob + q32 * p.C, p.C, nq, 32, sDh, sDl, lane, 64);
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
    wave_lds_sync();
    f32x4 pr[2][4], ds[2][4];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      u16x8 fqh[2], fql[2], fdh[2], fdl[2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        fqh[kk] = frag_rows(sQh, 16 * qt, kk, g, l15);
        fql[kk] = frag_rows(sQl, 16 * qt, kk, g, l15);
        fdh[kk] = frag_rows(sDh, 16 * qt, kk, g, l15);
        fdl[kk] = frag_rows(sDl, 16 * qt, kk, g, l15);
      }
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, d = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          s = mfma_x3(fqh[kk], fql[kk], frag_rows(sKh, 16 * kt, kk, g, l15), frag_rows(sKl, 16 * kt, kk, g, l15), s);
          d = mfma_x3(fdh[kk], fdl[kk], frag_rows(sVh, 16 * kt, kk, g, l15), frag_rows(sVl, 16 * kt, kk, g, l15), d);
        }
        const bool live = 16 * kt + l15 < nkeys;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pv = live ? __expf(s[r] * p.scale - lse[qt][r]) : 0.f;
          pr[qt][kt][r] = pv;
          ds[qt][kt][r] = p.scale * pv * (d[r] - dd[qt][r]);
        }
      }
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const u16x8 fdoTh = frag_cols(sDh, 4 * g, 16 + 4 * g, dt, l15), fdoTl = frag_cols(sDl, 4 * g, 16 + 4 * g, dt, l15);
      const u16x8 fqTh = frag_cols(sQh, 4 * g, 16 + 4 * g, dt, l15), fqTl = frag_cols(sQl, 4 * g, 16 + 4 * g, dt, l15);
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        u16x8 ph, pl, dh, dl;
        pack_pair_x3(pr[0][kt], pr[1][kt], ph, pl);
        pack_pair_x3(ds[0][kt], ds[1][kt], dh, dl);
        dvacc[dt][kt] = mfma_x3(fdoTh, fdoTl, ph, pl, dvacc[dt][kt]);
        dkacc[dt][kt] = mfma_x3(fqTh, fqTl, dh, dl, dkacc[dt][kt]);
      }
    }
  }
  // ---- fold the four waves' partials through LDS ([key][d], pitch 68), then store (direct mode) or one atomic per element
  __syncthreads();  // every wave is done with its staging tiles (the buffer is reused)
  float* red = reinterpret_cast<float*>(sbuf);
  for (int w = 0; w < NW; ++w) {
    if (wid == w) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          float* rk = red + (16 * kt + l15) * kRedPitch + 16 * dt + 4 * g;
          float* rv = rk + kKS * kRedPitch;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            rk[r] = (w ? rk[r] : 0.f) + dkacc[dt][kt][r];
            rv[r] = (w ? rv[r] : 0.f) + dvacc[dt][kt][r];
          }
        }
    }
    __syncthreads();
  }
  if (p.dkv_direct) {
    float* ob = p.dkv_direct + ((long)b * p.Nk + key0) * 2 * p.C + h * kHD;
    for (int e = tid; e < kKS * kHD; e += 64 * NW) {
      const int kl = e >> 6, d = e & 63;
      if (kl < nkeys) {
        ob[(long)kl * 2 * p.C + d] = red[kl * kRedPitch + d];
        ob[(long)kl * 2 * p.C + p.C + d] = red[(kKS + kl) * kRedPitch + d];
      }
    }
    return;
  }
  float* ob = p.dkv32 + ((long)b * p.Nk + key0) * 2 * p.C + h * kHD;
  for (int e = tid; e < kKS * kHD; e += 64 * NW) {
    const int kl = e >> 6, d = e & 63;
    if (kl < nkeys) {
      atomicAdd(ob + (long)kl * 2 * p.C + d, red[kl * kRedPitch + d]);
      atomicAdd(ob + (long)kl * 2 * p.C + p.C + d, red[(kKS + kl) * kRedPitch + d]);
    }
  }
}

}  // namespace

// head dim C / heads: 64 (the kernels above) or a larger multiple of 64 up to 1024 (attention_wide.hip)
static inline bool head_dim_ok(int heads, int C) {
  const int hd = C / heads;
  return C == heads * hd && hd % kHD == 0 && hd >= kHD && hd <= 1024;
}

// the full-key instances (attn_fwd_kernel<AttnBf16, 256, true>, attn_bwd_dq_kernel<AttnBf16, true>) take the launch when every one of the
// 256 key rows is live and the scale is positive (they take the row max over the raw scores); everything else -- a NaN scale too -- stays masked
static inline bool attn_full_keys(int Nk, float scale) { return Nk == kMaxK && scale > 0.f; }

// p: pointers, sizes and scale filled in by the C entry (arguments checked there), q_per_block chosen here
template <class Prec>
static int attn_fwd_launch(AttnParams<Prec> p, void* stream) {
  const bool full = Prec::P == 1 && attn_full_keys(p.Nk, p.scale);  // the bf16 kernels alone have full-key instances
  const int qpb = p.q_per_block = fwd_queries_per_block<Prec>(p.B, p.N, p.heads, full);
  const long nblk = (long)((p.N + qpb - 1) / qpb) * p.heads * p.B;
  if (nblk > 0x7fffffffL) return CMDA_ERR_SHAPE;
  dim3 grid((unsigned)nblk);
  if constexpr (Prec::P == 1) {
    if (full) CMDA_LAUNCH((attn_fwd_kernel<Prec, kMaxK, true>), grid, dim3(256), 0, stream, p);
    else if (p.Nk <= kMaxK) CMDA_LAUNCH((attn_fwd_kernel<Prec, kMaxK>), grid, dim3(256), 0, stream, p);
    else CMDA_LAUNCH((attn_fwd_kernel<Prec, kMaxKFwd>), grid, dim3(256), 0, stream, p);
  } else {
    CMDA_LAUNCH((attn_fwd_kernel<Prec, kMaxK>), grid, dim3(256), 0, stream, p);
  }
  CMDA_CHECK_LAUNCH();
}

// q [B*N, C] bf16, kv [B*Nk, 2C] bf16 -> o [B*N, C] bf16; head_dim = C / heads in {64, 128, ..., 1024}, Nk <= 320 (the backward: 256).
extern "C" int cmda_attention_fwd(const void* q, const void* kv, void* o, int B, int N, int Nk, int heads, int C,
                                  float scale, int dtype, void* stream) {
  if (B <= 0 || N <= 0) return CMDA_OK;
  if (dtype != CMDA_BF16) return CMDA_ERR_DTYPE;
  if (heads <= 0 || Nk <= 0 || Nk > kMaxKFwd || !head_dim_ok(heads, C)) return CMDA_ERR_UNSUPPORTED;
  if (heads > 65535 || B > 65535) return CMDA_ERR_SHAPE;
  if (C != heads * kHD) return attn_wide_fwd(q, kv, o, B, N, Nk, heads, C, scale, stream);
  return attn_fwd_launch(AttnParams<AttnBf16>{(const bf16_t*)q, {(const bf16_t*)kv}, (bf16_t*)o, B, N, Nk, heads, C, scale, 0}, stream);
}

// d_o [B*N, C] bf16 -> dq [B*N, C] bf16 (written), dkv32 [B*Nk, 2C] fp32 (accumulated: dK | dV; required when head_dim > 64).
// stats: scratch of cmda_attention_bwd_ws_floats(B, N, heads) floats.
extern "C" int64_t cmda_attention_bwd_ws_floats(int B, int N, int heads) { return (int64_t)B * N * heads * 2; }

// direct mode: with at most 1024 queries per (batch, head) ONE block per 64-key slice walks all of them, so dK | dV need no
// cross-block accumulation: they are stored as bf16 into dkv16 (no fp32 workspace, no atomics -- ~12 of the kernel's ~24 us at the
// stage-3 shape -- and no cast pass afterwards).  1 = cmda_attention_bwd will take dkv16 for these sizes.
extern "C" int cmda_attention_bwd_direct(int B, int N, int Nk, int heads) {
  (void)B; (void)heads;
  return N <= 1024 && Nk <= kMaxK ? 1 : 0;
}

// p: pointers (dkv_direct as the caller gave it), sizes and scale filled in by the C entry; launch geometry chosen here
template <class Prec>
static int attn_bwd_launch(AttnBwdParams<Prec> p, void* stream) {
  const int B = p.B, N = p.N, Nk = p.Nk, heads = p.heads;
  const bool direct = cmda_attention_bwd_direct(B, N, Nk, heads) != 0 && p.dkv_direct != nullptr;
  if (!direct && p.dkv32 == nullptr) return CMDA_ERR_SHAPE;
  if (!direct) p.dkv_direct = nullptr;
  const bool full = Prec::P == 1 && attn_full_keys(Nk, p.scale);
  const int fqpb = p.fwd_q_per_block = fwd_queries_per_block<Prec>(B, N, heads, full);
  const long nblk1 = (long)((N + fqpb - 1) / fqpb) * heads * B;
  if (nblk1 > 0x7fffffffL) return CMDA_ERR_SHAPE;
  dim3 g1((unsigned)nblk1);
  if constexpr (Prec::P == 1) {
    if (full) CMDA_LAUNCH((attn_bwd_dq_kernel<Prec, true>), g1, dim3(256), 0, stream, p);
    else CMDA_LAUNCH(attn_bwd_dq_masked_kernel, g1, dim3(256), 0, stream, p);
  } else {
    CMDA_LAUNCH((attn_bwd_dq_kernel<Prec, false>), g1, dim3(256), 0, stream, p);
  }
  // dK/dV: (batch, head, key slice) x query spans, spans a multiple of 128 queries.  Every span costs one fp32 atomic per
  // dK/dV element (~1.3 TB/s chip-wide: 1280 blocks of the stage-3 shape spent 31 of their 61 us there), so only as many
  // spans as it takes to reach ~2 blocks per CU -- and a single span (direct mode) when the queries are few.
  const long slices = (long)B * heads * ((Nk + kKS - 1) / kKS);
  long spans = direct ? 1 : std::max<long>(1, Prec::kSpanTarget / slices);
  long qpb = ((N + spans - 1) / spans + 127) / 128 * 128;
  spans = (N + qpb - 1) / qpb;
  p.q_per_block = (int)qpb;
  p.spans = (int)spans;
  dim3 g2((unsigned)(spans * heads * 4 * B));
  if constexpr (Prec::P == 1) {
    if (direct && N > 512) CMDA_LAUNCH((attn_bwd_dkv_kernel<Prec, 8>), g2, dim3(512), 0, stream, p);   // (N = 256: 21.4 us against 20.4 with 4 waves)
    else CMDA_LAUNCH((attn_bwd_dkv_kernel<Prec, 4>), g2, dim3(256), 0, stream, p);
  } else {
    CMDA_LAUNCH(attn_bwd_dkv_x3_kernel, g2, dim3(256), 0, stream, p);
  }
  CMDA_CHECK_LAUNCH();
}

extern "C" int cmda_attention_bwd(const void* q, const void* kv, const void* d_o, void* dq, float* dkv32, void* dkv16,
                                  float* stats, int B, int N, int Nk, int heads, int C, float scale, int dtype, void* stream) {
  if (B <= 0 || N <= 0) return CMDA_OK;
  if (dtype != CMDA_BF16) return CMDA_ERR_DTYPE;
  if (heads <= 0 || Nk <= 0 || Nk > kMaxK || !head_dim_ok(heads, C)) return CMDA_ERR_UNSUPPORTED;
  if (heads * 4 > 65535 || B > 65535) return CMDA_ERR_SHAPE;
  if (C != heads * kHD) {  // wide heads: accumulating form only (cmda_attention_bwd_direct knows no head dim)
    if (dkv32 == nullptr) return CMDA_ERR_SHAPE;
    return attn_wide_bwd(q, kv, d_o, dq, dkv32, stats, B, N, Nk, heads, C, scale, stream);
  }
  return attn_bwd_launch(AttnBwdParams<AttnBf16>{(const bf16_t*)q, {(const bf16_t*)kv}, (const bf16_t*)d_o, (bf16_t*)dq, dkv32, (bf16_t*)dkv16,
                                                 stats, B, N, Nk, heads, C, 0, scale, 0, 0},
                         stream);
}

// ---- split-bf16 instances (fp32 storage): q / o / d_o / dq / dK | dV fp32; kv_hi / kv_lo = cmda_split_bf16 of the fp32 [B*Nk, 2C] kv
extern "C" int cmda_attention_fwd_x3(const float* q, const void* kv_hi, const void* kv_lo, float* o, int B, int N, int Nk, int heads, int C,
                                     float scale, void* stream) {
  if (B <= 0 || N <= 0) return CMDA_OK;
  if (heads <= 0 || C != heads * kHD || Nk <= 0 || Nk > kMaxK || (C & 3)) return CMDA_ERR_UNSUPPORTED;
  if (heads > 65535 || B > 65535) return CMDA_ERR_SHAPE;
  return attn_fwd_launch(AttnParams<AttnSplit>{q, {(const bf16_t*)kv_hi, (const bf16_t*)kv_lo}, o, B, N, Nk, heads, C, scale, 0}, stream);
}

extern "C" int cmda_attention_bwd_x3(const float* q, const void* kv_hi, const void* kv_lo, const float* d_o, float* dq, float* dkv32,
                                     float* dkv_direct, float* stats, int B, int N, int Nk, int heads, int C, float scale, void* stream) {
  if (B <= 0 || N <= 0) return CMDA_OK;
  if (heads <= 0 || C != heads * kHD || Nk <= 0 || Nk > kMaxK || (C & 3)) return CMDA_ERR_UNSUPPORTED;
  if (heads * 4 > 65535 || B > 65535) return CMDA_ERR_SHAPE;
  return attn_bwd_launch(AttnBwdParams<AttnSplit>{q, {(const bf16_t*)kv_hi, (const bf16_t*)kv_lo}, d_o, dq, dkv32, dkv_direct, stats,
                                                  B, N, Nk, heads, C, 0, scale, 0, 0},
                         stream);
}
