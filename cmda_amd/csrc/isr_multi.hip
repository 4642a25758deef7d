// isr_multi.hip -- C ISR channels (one parameter row each: threshold, clip range, shifts) of one gray map, with an optional per-sample
// crop / flip window on the output (fourth ABI extension, include/cmda_hip_ext4.h).  The reference builds its three-channel ISR by
// calling get_image_change_from_pil three times on the host (cityscapes_ic.py:225-230, dark_zurich_ic.py:236-244, dacs.py:746-751);
// here it is three launches for the whole batch:
//   init   : the min / max records;
//   minmax : every thread reads a gray pixel once and forms all C x ndir shifted differences from it; per variant the four extremes
//            are reduced over the wave, the workgroup, then ONE integer atomic each (non-negative floats order like their bits);
//   apply  : C distinct planes, the window and the flip folded into the addressing.  The extremes are those of the WHOLE map.
// The arithmetic is isr_common.h's, shared with cmda_isr_from_gray: a channel is bit-identical to that entry point's output.
#include "isr_common.h"
#include "../../include/cmda_hip_ext4.h"

namespace {

constexpr int kMaxC = CMDAX4_ISR_MAX_C, kMaxDir = 4, kRow = CMDAX4_ISR_ROW, kThreads = 256;

static __device__ __forceinline__ int row_ndir(const int* __restrict__ row) { return row[2] == 4 ? 4 : 2; }

// mm[b][c][dir][4]: pos_min, pos_max, negabs_min, negabs_max
__global__ void __launch_bounds__(kThreads)
isr_multi_minmax_kernel(const unsigned char* __restrict__ gray, const float* __restrict__ lut, const int* __restrict__ prm,
                        unsigned* __restrict__ mm, int C, int H, int W) {
  __shared__ unsigned red[kThreads / 64][kMaxC * kMaxDir][4];
  const int b = blockIdx.y;
  const unsigned char* g = gray + (long)b * H * W;
  float st[kMaxC * kMaxDir][4];
#pragma unroll
  for (int v = 0; v < kMaxC * kMaxDir; ++v) { st[v][0] = INFINITY; st[v][1] = 0.f; st[v][2] = INFINITY; st[v][3] = 0.f; }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < H * W; i += gridDim.x * blockDim.x) {
    const int y = i / W, x = i - y * W;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) {
      if (c >= C) continue;
      const int* row = prm + c * kRow;
      const float thr = __int_as_float(row[0]), clip = __int_as_float(row[1]);
      const int nd = row_ndir(row);
#pragma unroll
      for (int dir = 0; dir < kMaxDir; ++dir) {
        if (dir >= nd) continue;
        const float d = isr_diff(g, lut, y, x, H, W, row[3 + 2 * dir], row[4 + 2 * dir], thr);
        const float pos = fminf(fmaxf(d, 0.f), clip);
        const float na = fminf(fmaxf(-d, 0.f), clip);  // |negative part|
        float* s = st[c * kMaxDir + dir];
        s[0] = fminf(s[0], pos); s[1] = fmaxf(s[1], pos);
        s[2] = fminf(s[2], na); s[3] = fmaxf(s[3], na);
      }
    }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int v = 0; v < kMaxC * kMaxDir; ++v) {
    if (v >= C * kMaxDir) continue;   // (uniform)
    const float a = wave_min(st[v][0]), bq = wave_max(st[v][1]), c = wave_min(st[v][2]), dd = wave_max(st[v][3]);
    if (lane == 0) {
      red[wid][v][0] = __float_as_uint(a); red[wid][v][1] = __float_as_uint(bq);
      red[wid][v][2] = __float_as_uint(c); red[wid][v][3] = __float_as_uint(dd);
    }
  }
  __syncthreads();
  // one thread per (variant, statistic): 48 at most
  const int t = threadIdx.x;
  if (t < C * kMaxDir * 4) {
    const int v = t >> 2, k = t & 3, c = v / kMaxDir, dir = v - c * kMaxDir;
    if (dir < row_ndir(prm + c * kRow)) {
      unsigned r = red[0][v][k];
      for (int w = 1; w < kThreads / 64; ++w) r = (k & 1) ? max(r, red[w][v][k]) : min(r, red[w][v][k]);
      unsigned* o = mm + (((long)b * C + c) * kMaxDir + dir) * 4 + k;
      if (k & 1) atomicMax(o, r); else atomicMin(o, r);
    }
  }
}

// out: NCHW fp32 [B,C,OH,OW]; win: [B][3] = {x0, y0, flip} or null
__global__ void isr_multi_apply_kernel(const unsigned char* __restrict__ gray, const float* __restrict__ lut,
                                       const int* __restrict__ prm, const int* __restrict__ win, const unsigned* __restrict__ mm,
                                       float* __restrict__ out, int B, int C, int H, int W, int OH, int OW) {
#pragma clang fp contract(off)
  const long OHW = (long)OH * OW, total = (long)B * OHW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / OHW);
    const int p = (int)(i - (long)b * OHW);
    const int oy = p / OW, ox = p - oy * OW;
    int y = oy, x = ox;
    if (win != nullptr) {
      const int x0 = min(max(win[3 * b], 0), W - OW), y0 = min(max(win[3 * b + 1], 0), H - OH);
      y = y0 + oy;
      x = x0 + (win[3 * b + 2] != 0 ? OW - 1 - ox : ox);
    }
    const unsigned char* g = gray + (long)b * H * W;
    for (int c = 0; c < C; ++c) {
      const int* row = prm + c * kRow;
      const float thr = __int_as_float(row[0]), clip = __int_as_float(row[1]);
      const int nd = row_ndir(row);
      const float share = 1.f / (float)nd;
      float acc = 0.f;
      for (int dir = 0; dir < nd; ++dir) {
        const float d = isr_diff(g, lut, y, x, H, W, row[3 + 2 * dir], row[4 + 2 * dir], thr);
        acc += isr_norm(d, clip, mm + (((long)b * C + c) * kMaxDir + dir) * 4) * share;
      }
      out[((long)b * C + c) * OHW + p] = acc;
    }
  }
}

static inline int grid_for(long n) { return (int)std::max<long>(1, std::min<long>((n + 255) / 256, 8192)); }
}  // namespace

extern "C" int cmdax4_abi_version(void) { return 1; }

extern "C" int cmdax4_isr_multi(const uint8_t* gray, const float* lut, const int32_t* prm, const int32_t* win, uint32_t* mm, float* out,
                                const int* ndir_check, const int* win_check, int B, int C, int H, int W, int OH, int OW, void* stream) {
  if (C < 1 || C > kMaxC || B < 0 || H < 1 || W < 1 || OH < 1 || OW < 1 || OH > H || OW > W) return CMDA_ERR_SHAPE;
  if (win == nullptr && (OH != H || OW != W)) return CMDA_ERR_SHAPE;
  if ((long)B * C * OH * OW >= (1L << 31) || (long)B * H * W >= (1L << 31)) return CMDA_ERR_SHAPE;
  if (ndir_check != nullptr)
    for (int c = 0; c < C; ++c)
      if (ndir_check[c] != 2 && ndir_check[c] != 4) return CMDA_ERR_SHAPE;
  if (win_check != nullptr)
    for (int b = 0; b < B; ++b) {
      const int x0 = win_check[3 * b], y0 = win_check[3 * b + 1], f = win_check[3 * b + 2];
      if (x0 < 0 || y0 < 0 || x0 > W - OW || y0 > H - OH || (f != 0 && f != 1)) return CMDA_ERR_SHAPE;
    }
  if (!gray || !lut || !prm || !mm || !out) return CMDA_ERR_UNSUPPORTED;
  if (B == 0) return CMDA_OK;
  const int nrec = B * C * kMaxDir;
  CMDA_LAUNCH(minmax_init_kernel, dim3((nrec * 4 + 255) / 256), dim3(256), 0, stream, (unsigned*)mm, nrec);
  dim3 grid(std::max(1, std::min((H * W + kThreads - 1) / kThreads, 256)), B);
  CMDA_LAUNCH(isr_multi_minmax_kernel, grid, dim3(kThreads), 0, stream, (const unsigned char*)gray, lut, (const int*)prm,
              (unsigned*)mm, C, H, W);
  CMDA_LAUNCH(isr_multi_apply_kernel, dim3(grid_for((long)B * OH * OW)), dim3(256), 0, stream, (const unsigned char*)gray, lut,
              (const int*)prm, (const int*)win, (const unsigned*)mm, out, B, C, H, W, OH, OW);
  CMDA_CHECK_LAUNCH();
}
