// voxel_ordered.hip -- the event tail of the DSEC target loader, batched and bit-reproducible (include/cmda_hip_ext5.h, `cmdax5_`).
//
// (1) event_prep_batch : cmda_event_prep (pipeline.hip) for B concatenated samples in one launch.
// (2) voxel_ordered    : events_to_voxel_grid (mmseg/datasets/dsec.py:26-70) WITHOUT float atomics.  The reference adds the
//     contributions of a cell sequentially in fp32 (eight put_(accumulate=True) passes, one per corner, each in event order), so
//     the sum has ONE right answer per cell and an order-preserving kernel reproduces it bit for bit.  Store-then-sum through an
//     inverted index:
//       count  : contributions per cell (integer atomics)
//       scan   : exclusive scan over the cells of a sample -> segment starts (tile sums, scan of the sums, apply)
//       fill   : every contribution drops a 64-bit record (order key  corner * N_b + i, weight) into its cell's segment through
//                an integer atomic cursor (the position inside the segment is arbitrary, the KEY carries the order); the cursor
//                array ends up holding the segment ends, so one array serves as count, start and end
//       sum    : per cell, add the weights in ascending key order; the segment is contiguous, the event arrays are not read again.
//                <= 32 records: one lane, by repeated selection of the next larger key (no writes, L*L reads of a cached segment);
//                longer      : listed, and one workgroup per listed cell sorts the records (all-ascending bitonic network: in LDS
//                              up to 4096 records, in the record buffer itself beyond) and one lane adds the weights in order.
//                              Per-cell work is O(L log^2 L / 256) + L for any L.
// (3) events_norm_batch: events_norm (dsec.py:80-121) for B grids; count / sum / sum of squares as stored per-workgroup partials
//     added in index order (no float / double atomics), min / max through integer atomics as in extractors.hip.
// Per-sample host data (offsets, clip ranges) reach the kernels as by-value launch arguments (at most CMDAX5_MAX_B samples).
#include "common.h"
#include "../../include/cmda_hip_ext5.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSmall = CMDAX5_SMALL_SEGMENT;
constexpr int kLdsRecs = 4096;                       // 32 KiB of LDS
constexpr int kScanPer = CMDAX5_SCAN_TILE / kThreads;  // cells per thread of a scan tile
constexpr int kLongBlocks = 1024;

struct Offsets { long long v[CMDAX5_MAX_B + 1]; };
struct Clips { float v[CMDAX5_MAX_B]; };

static inline int grid_for(long n, int cap) { return (int)std::max<long>(1, std::min<long>((n + kThreads - 1) / kThreads, cap)); }

// ---------------------------------------------------------------------------------------------------- event prep
__global__ void event_prep_batch_kernel(const long long* __restrict__ t, const int* __restrict__ x, const int* __restrict__ y,
                                        const unsigned char* __restrict__ p, Offsets offs, const float* __restrict__ rect_map, int W,
                                        float* __restrict__ tn, float* __restrict__ xr, float* __restrict__ yr,
                                        float* __restrict__ pol) {
#pragma clang fp contract(off)
  const long s = offs.v[blockIdx.y], e = offs.v[blockIdx.y + 1];
  if (e <= s) return;
  const long long t0 = t[s];
  const float tlast = (float)(t[e - 1] - t0);
  for (long i = s + (long)blockIdx.x * blockDim.x + threadIdx.x; i < e; i += (long)gridDim.x * blockDim.x) {
    tn[i] = (float)(t[i] - t0) / tlast;
    pol[i] = (float)p[i];
    const int xi = x[i], yi = y[i];
    if (rect_map) {
      const float* m = rect_map + ((long)yi * W + xi) * 2;
      xr[i] = m[0];
      yr[i] = m[1];
    } else {
      xr[i] = (float)xi;
      yr[i] = (float)yi;
    }
  }
}

// ---------------------------------------------------------------------------------------------------- voxel grid
// One event as voxel_scatter_kernel (extractors.hip) sees it; corner = 4*ax + 2*ay + at.
struct Event {
  float tn, xv, yv, value;
  int x0, y0, tb;
};

static __device__ __forceinline__ Event load_event(const float* __restrict__ t, const float* __restrict__ x,
                                                   const float* __restrict__ y, const float* __restrict__ pol, long i, float t0,
                                                   float tN, int C) {
#pragma clang fp contract(off)
  Event e;
  e.tn = (float)(C - 1) * (t[i] - t0) / (tN - t0);
  e.xv = x[i];
  e.yv = y[i];
  e.x0 = (int)e.xv;
  e.y0 = (int)e.yv;
  e.tb = (int)e.tn;
  e.value = 2.f * pol[i] - 1.f;
  return e;
}

static __device__ __forceinline__ bool corner_cell(const Event& e, int corner, int C, int H, int W, int& cell) {
  const int xl = e.x0 + (corner >> 2), yl = e.y0 + ((corner >> 1) & 1), tl = e.tb + (corner & 1);
  cell = (tl * H + yl) * W + xl;  // used only when inside
  return xl < W && xl >= 0 && yl < H && yl >= 0 && tl >= 0 && tl < C;
}

static __device__ __forceinline__ float corner_weight(const Event& e, int corner) {
#pragma clang fp contract(off)
  const int xl = e.x0 + (corner >> 2), yl = e.y0 + ((corner >> 1) & 1), tl = e.tb + (corner & 1);
  return e.value * (1.f - fabsf((float)xl - e.xv)) * (1.f - fabsf((float)yl - e.yv)) * (1.f - fabsf((float)tl - e.tn));
}

// The events of one sample.
struct Sample {
  const float *t, *x, *y, *pol;
  float t0, tN;
  unsigned n;
};

static __device__ __forceinline__ Sample sample_of(const float* t, const float* x, const float* y, const float* pol, long s, long e) {
  Sample sm;
  sm.t = t + s; sm.x = x + s; sm.y = y + s; sm.pol = pol + s;
  sm.n = (unsigned)(e - s);
  sm.t0 = sm.t[0]; sm.tN = sm.t[sm.n - 1];
  return sm;
}

// One contribution as it waits in its cell's segment: the order key corner * N_b + i (plus one, so that no record is 0) in the
// high word, the weight's bit pattern in the low word.  Keys are distinct inside a cell, so records order like their keys.
typedef unsigned long long rec_t;
static __device__ __forceinline__ rec_t make_rec(unsigned key, float w) { return ((rec_t)(key + 1u) << 32) | __float_as_uint(w); }
static __device__ __forceinline__ float rec_weight(rec_t r) { return __uint_as_float((unsigned)r); }

// zero the counters (cells + the long-cell counter) and put the offsets on the device
__global__ void vo_init_kernel(unsigned* __restrict__ cnt, long nwords, long long* __restrict__ offs_dev, Offsets offs, int B) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += (long)gridDim.x * blockDim.x) cnt[i] = 0u;
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i <= B; i += blockDim.x) offs_dev[i] = offs.v[i];
}

// FILL = false: count the contributions per cell; FILL = true: cnt holds the segment starts and works as a cursor
template <bool FILL>
__global__ void vo_scatter_kernel(const float* __restrict__ t, const float* __restrict__ x, const float* __restrict__ y,
                                  const float* __restrict__ pol, const long long* __restrict__ offs, unsigned* __restrict__ cnt,
                                  rec_t* __restrict__ recs, int C, int H, int W) {
  const int b = blockIdx.y;
  const long s = offs[b], e = offs[b + 1];
  if (e <= s) return;
  const Sample sm = sample_of(t, x, y, pol, s, e);
  unsigned* c = cnt + (long)b * C * H * W;
  rec_t* r = recs + 8 * s;  // a sample's records: at most eight per event
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < sm.n; i += gridDim.x * blockDim.x) {
    const Event ev = load_event(sm.t, sm.x, sm.y, sm.pol, (long)i, sm.t0, sm.tN, C);
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
      int cell;
      if (corner_cell(ev, corner, C, H, W, cell)) {
        const unsigned pos = atomicAdd(c + cell, 1u);
        if (FILL) r[pos] = make_rec((unsigned)corner * sm.n + i, corner_weight(ev, corner));
      }
    }
  }
}

// exclusive scan of one value per thread over the workgroup; sh: kThreads words
static __device__ __forceinline__ unsigned block_scan_excl(unsigned v, unsigned* sh, unsigned& total) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int o = 1; o < kThreads; o <<= 1) {
    const unsigned a = tid >= o ? sh[tid - o] : 0u;
    __syncthreads();
    sh[tid] += a;
    __syncthreads();
  }
  const unsigned incl = sh[tid];
  total = sh[kThreads - 1];
  __syncthreads();
  return incl - v;
}

// scan, step 1: the sum of every tile of CMDAX5_SCAN_TILE cells -> part[b][tile]
__global__ void vo_scan_sums_kernel(const unsigned* __restrict__ cnt, unsigned* __restrict__ part, long cps, int ntile) {
  __shared__ unsigned sh[kThreads];
  const unsigned* c = cnt + (long)blockIdx.y * cps;
  const long base = (long)blockIdx.x * CMDAX5_SCAN_TILE;
  unsigned v = 0;
  for (int k = 0; k < kScanPer; ++k) {
    const long i = base + k * kThreads + threadIdx.x;
    if (i < cps) v += c[i];
  }
  unsigned total;
  block_scan_excl(v, sh, total);
  if (threadIdx.x == 0) part[(long)blockIdx.y * ntile + blockIdx.x] = total;
}

// scan, step 2: exclusive scan of a sample's tile sums in place (one workgroup per sample)
__global__ void vo_scan_parts_kernel(unsigned* __restrict__ part, int ntile) {
  __shared__ unsigned sh[kThreads];
  unsigned* p = part + (long)blockIdx.x * ntile;
  const int per = (ntile + kThreads - 1) / kThreads;
  const int lo = min(threadIdx.x * per, (unsigned)ntile), hi = min(lo + per, ntile);
  unsigned v = 0;
  for (int i = lo; i < hi; ++i) v += p[i];
  unsigned total;
  unsigned run = block_scan_excl(v, sh, total);
  for (int i = lo; i < hi; ++i) {
    const unsigned here = p[i];
    p[i] = run;
    run += here;
  }
}

// scan, step 3: counts -> segment starts (relative to the sample's first key)
__global__ void vo_scan_apply_kernel(unsigned* __restrict__ cnt, const unsigned* __restrict__ part, long cps, int ntile) {
  __shared__ unsigned sh[kThreads];
  __shared__ unsigned tile[CMDAX5_SCAN_TILE];
  unsigned* c = cnt + (long)blockIdx.y * cps;
  const long base = (long)blockIdx.x * CMDAX5_SCAN_TILE;
  for (int k = 0; k < kScanPer; ++k) {
    const long i = base + k * kThreads + threadIdx.x;
    tile[k * kThreads + threadIdx.x] = i < cps ? c[i] : 0u;
  }
  __syncthreads();
  unsigned v = 0;
  for (int k = 0; k < kScanPer; ++k) v += tile[threadIdx.x * kScanPer + k];
  unsigned total;
  unsigned run = block_scan_excl(v, sh, total) + part[(long)blockIdx.y * ntile + blockIdx.x];
  for (int k = 0; k < kScanPer; ++k) {
    const unsigned here = tile[threadIdx.x * kScanPer + k];
    tile[threadIdx.x * kScanPer + k] = run;
    run += here;
  }
  __syncthreads();
  for (int k = 0; k < kScanPer; ++k) {
    const long i = base + k * kThreads + threadIdx.x;
    if (i < cps) c[i] = tile[k * kThreads + threadIdx.x];
  }
}

// After the fill, cnt[c] is the END of cell c's segment; it starts where its predecessor ends.
static __device__ __forceinline__ void segment_of(const unsigned* __restrict__ c, long cell, unsigned& start, unsigned& len) {
  start = cell > 0 ? c[cell - 1] : 0u;
  len = c[cell] - start;
}

// sum, short segments: one lane per cell; longer ones are listed for vo_sum_long_kernel
__global__ void vo_sum_small_kernel(const long long* __restrict__ offs, const unsigned* __restrict__ cnt,
                                    const rec_t* __restrict__ recs, unsigned* __restrict__ nlong, unsigned* __restrict__ longlist,
                                    float* __restrict__ grid, long cps) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const unsigned* c = cnt + (long)b * cps;
  const rec_t* r = recs + 8 * offs[b];
  float* g = grid + (long)b * cps;
  for (long cell = (long)blockIdx.x * blockDim.x + threadIdx.x; cell < cps; cell += (long)gridDim.x * blockDim.x) {
    unsigned start, len;
    segment_of(c, cell, start, len);
    if (len > (unsigned)kSmall) {
      longlist[atomicAdd(nlong, 1u)] = (unsigned)((long)b * cps + cell);
      continue;
    }
    float acc = 0.f;   // a sample without events has only empty segments: a zero grid
    rec_t last = 0;    // below every record
    for (unsigned done = 0; done < len; ++done) {
      rec_t next = ~(rec_t)0;  // above every record: keys stay below 8 * 2^29
      for (unsigned j = 0; j < len; ++j) {
        const rec_t v = r[start + j];
        if (v > last && v < next) next = v;
      }
      acc = acc + rec_weight(next);
      last = next;
    }
    g[cell] = acc;
  }
}

// All-ascending bitonic network over a[0..len): every comparator puts the smaller record at the lower index, so the positions
// len .. 2^k - 1 behave as +infinity that never moves and are simply skipped (the first stage of each merge mirrors the upper
// half, i ^ (k - 1), instead of reversing the direction of the comparators).  Called by the whole workgroup.
static __device__ __forceinline__ void workgroup_sort(rec_t* a, unsigned len) {
  unsigned pow2 = 1;
  while (pow2 < len) pow2 <<= 1;
  for (unsigned k = 2; k <= pow2; k <<= 1)
    for (unsigned j = k >> 1; j > 0; j >>= 1) {
      for (unsigned q = threadIdx.x; q < (pow2 >> 1); q += blockDim.x) {
        const unsigned lo = ((q & ~(j - 1)) << 1) | (q & (j - 1));   // comparator q: bit log2(j) of its lower index is 0
        const unsigned hi = j == (k >> 1) ? (lo ^ (k - 1)) : (lo | j);
        if (hi < len) {
          const rec_t u = a[lo], v = a[hi];
          if (u > v) { a[lo] = v; a[hi] = u; }
        }
      }
      __syncthreads();
    }
}

// sum, long segments: one workgroup per listed cell sorts the records (in LDS when they fit, in place otherwise), one lane adds
__global__ void vo_sum_long_kernel(const long long* __restrict__ offs, const unsigned* __restrict__ cnt, rec_t* recs,
                                   const unsigned* __restrict__ nlong, const unsigned* __restrict__ longlist,
                                   float* __restrict__ grid, long cps) {
#pragma clang fp contract(off)
  __shared__ rec_t buf[kLdsRecs];
  const unsigned n_listed = *nlong;
  for (unsigned item = blockIdx.x; item < n_listed; item += gridDim.x) {
    const long gcell = longlist[item];
    const int b = (int)(gcell / cps);
    unsigned start, len;
    segment_of(cnt + (long)b * cps, gcell - (long)b * cps, start, len);
    rec_t* seg = recs + 8 * offs[b] + start;
    rec_t* a = seg;
    if (len <= (unsigned)kLdsRecs) {
      for (unsigned i = threadIdx.x; i < len; i += blockDim.x) buf[i] = seg[i];
      __syncthreads();
      a = buf;
    }
    workgroup_sort(a, len);
    if (threadIdx.x == 0) {
      float acc = 0.f;
      for (unsigned i = 0; i < len; ++i) acc = acc + rec_weight(a[i]);
      grid[gcell] = acc;
    }
    __syncthreads();  // buf is reused by the next item
  }
}

// ---------------------------------------------------------------------------------------------------- events_norm
static __device__ __forceinline__ float events_standardise(float v, float mean, float stdv, int any) {  // as extractors.hip
  if (!any) return v;
  return (v != 0.f ? 1.f : 0.f) * (v - mean) / (stdv + 1e-8f);
}

// part[b][blk][3]: non-zero count, sum, sum of squares of the block's share; block 0 also initialises the sample's min / max record
__global__ void norm_stats_kernel(const float* __restrict__ ev, double* __restrict__ part, unsigned* __restrict__ mm, long n) {
  __shared__ double buf[kThreads][3];
  const float* e = ev + (long)blockIdx.y * n;
  double c = 0, s = 0, q = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = e[i];
    if (v != 0.f) c += 1.0;
    s += v;
    q += (double)v * v;
  }
  buf[threadIdx.x][0] = c; buf[threadIdx.x][1] = s; buf[threadIdx.x][2] = q;
  __syncthreads();
  if (threadIdx.x < 3) {
    double a = 0;
    for (int k = 0; k < kThreads; ++k) a += buf[k][threadIdx.x];
    part[((long)blockIdx.y * gridDim.x + blockIdx.x) * 3 + threadIdx.x] = a;
  }
  if (blockIdx.x == 0 && threadIdx.x < 4) mm[blockIdx.y * 4 + threadIdx.x] = (threadIdx.x & 1) ? 0u : 0x7F800000u;
}

// the partials of sample b added in index order: the same three sums in every workgroup that asks
static __device__ __forceinline__ void norm_totals(const double* __restrict__ part, int nparts, double* tot, int& any, float& mean,
                                                   float& stdv) {
  if (threadIdx.x < 3) {
    double a = 0;
    for (int k = 0; k < nparts; ++k) a += part[k * 3 + threadIdx.x];
    tot[threadIdx.x] = a;
  }
  __syncthreads();
  const double cnt = tot[0];
  any = cnt > 0;
  mean = any ? (float)(tot[1] / cnt) : 0.f;
  stdv = any ? sqrtf((float)(tot[2] / cnt) - mean * mean) : 1.f;
}

__global__ void norm_minmax_kernel(const float* __restrict__ ev, const double* __restrict__ part, unsigned* __restrict__ mm, long n,
                                   int nparts, Clips clips) {
  __shared__ double tot[3];
  __shared__ unsigned red[4][4];
  const int b = blockIdx.y;
  const float* e = ev + (long)b * n;
  const float clip = clips.v[b];
  int any;
  float mean, stdv;
  norm_totals(part + (long)b * nparts * 3, nparts, tot, any, mean, stdv);
  float pmin = INFINITY, pmax = 0.f, nmin = INFINITY, nmax = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = events_standardise(e[i], mean, stdv, any);
    const float pos = fminf(fmaxf(v, 0.f), clip), na = fminf(fmaxf(-v, 0.f), clip);
    pmin = fminf(pmin, pos); pmax = fmaxf(pmax, pos); nmin = fminf(nmin, na); nmax = fmaxf(nmax, na);
  }
  pmin = wave_min(pmin); pmax = wave_max(pmax); nmin = wave_min(nmin); nmax = wave_max(nmax);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    red[wid][0] = __float_as_uint(pmin); red[wid][1] = __float_as_uint(pmax);
    red[wid][2] = __float_as_uint(nmin); red[wid][3] = __float_as_uint(nmax);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned a = red[0][0], bq = red[0][1], c = red[0][2], d = red[0][3];
    for (int w = 1; w < 4; ++w) { a = min(a, red[w][0]); bq = max(bq, red[w][1]); c = min(c, red[w][2]); d = max(d, red[w][3]); }
    unsigned* o = mm + b * 4;
    atomicMin(o + 0, a); atomicMax(o + 1, bq); atomicMin(o + 2, c); atomicMax(o + 3, d);
  }
}

__global__ void norm_apply_kernel(const float* ev, const double* __restrict__ part, const unsigned* __restrict__ mm, float* out,
                                  long n, int nparts, Clips clips, float final_range) {
#pragma clang fp contract(off)
  __shared__ double tot[3];
  const int b = blockIdx.y;
  const float* e = ev + (long)b * n;
  float* o = out + (long)b * n;
  const float clip = clips.v[b];
  int any;
  float mean, stdv;
  norm_totals(part + (long)b * nparts * 3, nparts, tot, any, mean, stdv);
  const unsigned* m = mm + b * 4;
  const float pmin = __uint_as_float(m[0]), pmax = __uint_as_float(m[1]);
  const float nlo = -__uint_as_float(m[3]), nhi = -__uint_as_float(m[2]);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = events_standardise(e[i], mean, stdv, any);
    const float pos = fminf(fmaxf(v, 0.f), clip), neg = fminf(fmaxf(v, -clip), 0.f);
    const float pn = (pos - pmin) / (pmax - pmin + 1e-8f) * (final_range - 0.f) + 0.f;
    const float nn = (neg - nlo) / (nhi - nlo + 1e-8f) * (0.f - -final_range) + -final_range;
    o[i] = pn + nn;
  }
}

// ---------------------------------------------------------------------------------------------------- host side
// B and the offsets: CMDA_OK with the by-value copy filled, or the refusal
static int check_offsets(const int64_t* offsets, int B, Offsets& out) {
  if (B < 1 || B > CMDAX5_MAX_B) return CMDA_ERR_SHAPE;
  if (!offsets) return CMDA_ERR_UNSUPPORTED;
  if (offsets[0] != 0) return CMDA_ERR_SHAPE;
  for (int b = 0; b < B; ++b) {
    const int64_t n = offsets[b + 1] - offsets[b];
    if (n < 0 || n >= (int64_t)CMDAX5_MAX_EVENTS) return CMDA_ERR_SHAPE;
  }
  for (int b = 0; b <= B; ++b) out.v[b] = offsets[b];
  return CMDA_OK;
}

static inline long scan_tiles(long cps) { return (cps + CMDAX5_SCAN_TILE - 1) / CMDAX5_SCAN_TILE; }
static inline long long_list_cap(long cells, long n_total) { return std::min<long>(cells, 8 * n_total / (kSmall + 1)) + 1; }
static inline int norm_parts(long n) { return (int)std::min<long>(256, (n + CMDAX5_NORM_TILE - 1) / CMDAX5_NORM_TILE); }
}  // namespace

extern "C" int cmdax5_abi_version(void) { return 1; }

extern "C" int cmdax5_event_prep_batch(const int64_t* t, const int32_t* x, const int32_t* y, const uint8_t* p, const int64_t* offsets,
                                       int B, const float* rect_map, int H, int W, float* t_norm, float* xr, float* yr, float* pol,
                                       void* stream) {
  Offsets offs;
  if (H < 1 || W < 1) return CMDA_ERR_SHAPE;
  const int rc = check_offsets(offsets, B, offs);
  if (rc != CMDA_OK) return rc;
  const long n_total = (long)offs.v[B];
  if (n_total == 0) return CMDA_OK;
  if (!t || !x || !y || !p || !t_norm || !xr || !yr || !pol) return CMDA_ERR_UNSUPPORTED;
  long n_max = 0;
  for (int b = 0; b < B; ++b) n_max = std::max<long>(n_max, (long)(offs.v[b + 1] - offs.v[b]));
  CMDA_LAUNCH(event_prep_batch_kernel, dim3(grid_for(n_max, 4096), B), dim3(kThreads), 0, stream, (const long long*)t, x, y, p, offs,
              rect_map, W, t_norm, xr, yr, pol);
  CMDA_CHECK_LAUNCH();
}

extern "C" int64_t cmdax5_voxel_ordered_ws_bytes(int B, int64_t n_total, int bins, int H, int W) {
  if (B < 1 || B > CMDAX5_MAX_B || bins < 1 || H < 1 || W < 1 || n_total < 0) return 0;
  const int64_t cps = (int64_t)bins * H * W;
  if (cps >= (1ll << 31) || cps * B >= (1ll << 31) || n_total > (int64_t)B * (CMDAX5_MAX_EVENTS - 1)) return 0;
  const int64_t cells = cps * B;
  const int64_t bytes = 8 * (int64_t)(B + 1) + 4 * (cells + 2) + 4 * (int64_t)B * scan_tiles(cps) + 4 * long_list_cap(cells, n_total) +
                        64 * n_total;
  return (bytes + 7) / 8 * 8;
}

extern "C" int cmdax5_voxel_ordered(const float* t, const float* x, const float* y, const float* pol, const int64_t* offsets,
                                    float* grid, void* ws, int B, int bins, int H, int W, void* stream) {
  Offsets offs;
  if (bins < 1 || H < 1 || W < 1) return CMDA_ERR_SHAPE;
  const int rc = check_offsets(offsets, B, offs);
  if (rc != CMDA_OK) return rc;
  const long cps = (long)bins * H * W;
  if (cps >= (1l << 31) || cps * B >= (1l << 31)) return CMDA_ERR_SHAPE;
  const long cells = cps * B, n_total = (long)offs.v[B];
  if (!grid || !ws || (n_total > 0 && (!t || !x || !y || !pol))) return CMDA_ERR_UNSUPPORTED;
  const int ntile = (int)scan_tiles(cps);
  // the workspace, in the order of cmdax5_voxel_ordered_ws_bytes
  long long* offs_dev = (long long*)ws;
  rec_t* recs = (rec_t*)(offs_dev + B + 1);
  unsigned* cnt = (unsigned*)(recs + 8 * n_total);
  unsigned* nlong = cnt + cells;  // cnt[cells]; one word of padding follows
  unsigned* part = cnt + cells + 2;
  unsigned* longlist = part + (long)B * ntile;
  long n_max = 0;
  for (int b = 0; b < B; ++b) n_max = std::max<long>(n_max, (long)(offs.v[b + 1] - offs.v[b]));

  CMDA_LAUNCH(vo_init_kernel, dim3(grid_for(cells + 1, 1024)), dim3(kThreads), 0, stream, cnt, cells + 1, offs_dev, offs, B);
  const dim3 ev_grid(grid_for(std::max<long>(n_max, 1), 2048), B);
  CMDA_LAUNCH(vo_scatter_kernel<false>, ev_grid, dim3(kThreads), 0, stream, t, x, y, pol, (const long long*)offs_dev, cnt, recs, bins,
              H, W);
  CMDA_LAUNCH(vo_scan_sums_kernel, dim3(ntile, B), dim3(kThreads), 0, stream, (const unsigned*)cnt, part, cps, ntile);
  CMDA_LAUNCH(vo_scan_parts_kernel, dim3(B), dim3(kThreads), 0, stream, part, ntile);
  CMDA_LAUNCH(vo_scan_apply_kernel, dim3(ntile, B), dim3(kThreads), 0, stream, cnt, (const unsigned*)part, cps, ntile);
  CMDA_LAUNCH(vo_scatter_kernel<true>, ev_grid, dim3(kThreads), 0, stream, t, x, y, pol, (const long long*)offs_dev, cnt, recs, bins,
              H, W);
  CMDA_LAUNCH(vo_sum_small_kernel, dim3(grid_for(cps, 4096), B), dim3(kThreads), 0, stream, (const long long*)offs_dev,
              (const unsigned*)cnt, (const rec_t*)recs, nlong, longlist, grid, cps);
  CMDA_LAUNCH(vo_sum_long_kernel, dim3(kLongBlocks), dim3(kThreads), 0, stream, (const long long*)offs_dev, (const unsigned*)cnt,
              recs, (const unsigned*)nlong, (const unsigned*)longlist, grid, cps);
  CMDA_CHECK_LAUNCH();
}

extern "C" int64_t cmdax5_events_norm_ws_bytes(int B, int64_t n) {
  if (B < 1 || B > CMDAX5_MAX_B || n < 1 || n * B >= (1ll << 31)) return 0;
  return 24 * (int64_t)B * norm_parts(n) + 16 * (int64_t)B;
}

extern "C" int cmdax5_events_norm_batch(const float* events, float* out, void* ws, int B, int64_t n, const float* clip_ranges,
                                        float final_range, void* stream) {
  if (B < 1 || B > CMDAX5_MAX_B || n < 1 || n * B >= (1ll << 31)) return CMDA_ERR_SHAPE;
  if (!events || !out || !ws || !clip_ranges) return CMDA_ERR_UNSUPPORTED;
  Clips clips;
  for (int b = 0; b < B; ++b) clips.v[b] = clip_ranges[b];
  const int nparts = norm_parts(n);
  double* part = (double*)ws;
  unsigned* mm = (unsigned*)(part + (long)B * nparts * 3);
  CMDA_LAUNCH(norm_stats_kernel, dim3(nparts, B), dim3(kThreads), 0, stream, events, part, mm, (long)n);
  // few workgroups for the min / max pass: every one ends in four atomics on the sample's record, and 1024 of them per sample spent
  // 109 us queueing on those four words (16 us for the apply pass over the same data)
  CMDA_LAUNCH(norm_minmax_kernel, dim3(grid_for(n, 128), B), dim3(kThreads), 0, stream, events, (const double*)part, mm, (long)n,
              nparts, clips);
  const dim3 grid(grid_for(n, 1024), B);
  CMDA_LAUNCH(norm_apply_kernel, grid, dim3(kThreads), 0, stream, events, (const double*)part, (const unsigned*)mm, out, (long)n,
              nparts, clips, final_range);
  CMDA_CHECK_LAUNCH();
}
