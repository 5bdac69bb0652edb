// hopsx: what the validation pair rules read off two feature columns at once (gfx950): the moments behind a
// correlation, the row comparison counts, and the dense ranks behind a mutual information.
//
// x is fp64 [rows][cols], row-major, NaN = missing (the layout hopsx_column_sort64 takes); it is only read.  pairs is
// int32 [P][2], column indices (a, b); self pairs, both orders of a pair and one column in many pairs are all allowed.
//
//   hopsx_column_pair_moments64  per pair, over the rows where both values are non-NaN:
//                                counts[p] = n, #(a < b), #(a == b), #(a > b)
//                                sums[p]   = sum a, sum b, Saa, Sbb, Sab, the last three centred about the means
//   hopsx_column_pair_ranks64    comp[p][r] = rank_a << 32 | rank_b with rank_c the index of row r's sort key among the
//                                distinct keys of column c (NaN is one class, the last; -0.0 is +0.0: colsort.hip's keys),
//                                and dcount[c] = that column's distinct keys.  Sorted by hopsx_column_sort_keys64, the
//                                runs of comp[p] are the joint multiplicities of the pair.
//
// Moments: a workgroup owns a tile of kTile rows.  Up to kStageCols columns the tile is staged in LDS, read as the one
// contiguous block it is in x and written transposed; with more columns the lanes read x directly.  Waves take the
// pairs round-robin, lanes stride the tile's rows, fp64 accumulators in registers, integer counts from ballots, then
// the xor tree of the wave.  Every tile leaves one partial per pair and quantity; one workgroup per pair adds them,
// thread t the tiles t, t + 256, ... in turn, then a fixed tree.  Two passes: the first leaves n, the sums and the
// comparison counts, the second accumulates d = a - mean(a), e = b - mean(b) as sum d, sum e, sum d^2, sum e^2,
// sum d e, and Saa = sum d^2 - (sum d)^2 / n (clamped at 0) takes the rounding of the mean out again (likewise Sbb,
// Sab).  No float atomics: a partial depends on its tile alone, so the bits do not depend on the grid.
//
// Ranks: the distinct keys of every sorted column are compacted into a table (heads per tile of kCTile keys, a scan
// over the tiles, an ordered write).  A workgroup of rank_k serves one pair and walks rows grid-stride.  It stages both
// columns' tables once: a table of at most kTableKeys keys whole, a larger one as every s-th key (s = ceil(d /
// kTableKeys)).  A row's rank is a lower bound in LDS followed by a lower bound over the at most s - 1 keys between
// two samples in global memory; with s = 1 that second search is empty.
#include "common.h"
#include "ops_api.h"

namespace colpair {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / HOPSX_WAVE;
constexpr int kTile = 512;        // rows per tile of the moments kernels
constexpr int kStageCols = 16;    // columns staged: 16 x 512 doubles = 64 KiB
constexpr int kMomWords = 6;      // partials per pair and tile: pass 1 n, lt, eq, gt, sum a, sum b; pass 2 uses 5
constexpr int kPerThread = 8;
constexpr int kCTile = kThreads * kPerThread;  // keys per tile of the compaction
constexpr int kTableKeys = 2048;               // keys (or samples) of one column's table in LDS
constexpr int kDefaultGrid = 4096;
constexpr uint64_t kNaNKey = ~0ull;

// the key rule of colsort.hip
__device__ __forceinline__ uint64_t key_of(double v) {
  if (v != v) return kNaNKey;
  uint64_t k = (uint64_t)__double_as_longlong(v);
  if (k == 0x8000000000000000ull) k = 0ull;
  return (k >> 63) ? ~k : (k | 0x8000000000000000ull);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned popc(bool b) { return (unsigned)__popcll(__ballot(b)); }

static inline long tiles_of(long rows, int tile) { return (rows + tile - 1) / tile; }
static inline int grid_x(long ntiles, int g, int max_workgroups) {
  const long cap = max_workgroups > 0 ? max_workgroups : kDefaultGrid;
  long gx = cap / (g > 0 ? g : 1);
  if (gx < 1) gx = 1;
  if (gx > ntiles) gx = ntiles;
  return (int)gx;
}

// part[(p * kMomWords + q) * ntiles + tile]
template <int PASS>
__global__ __launch_bounds__(kThreads) void moments_k(const double* __restrict__ x, int rows, int cols,
                                                      const int* __restrict__ pairs, int P,
                                                      const long long* __restrict__ counts,
                                                      const double* __restrict__ sums, uint64_t* __restrict__ part) {
  __shared__ double sx[kStageCols * kTile];
  const bool staged = cols <= kStageCols;
  const long ntiles = ((long)rows + kTile - 1) / kTile;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long r0 = tile * kTile;
    const int nt = (int)(rows - r0 < kTile ? rows - r0 : kTile);
    if (staged) {
      const double* src = x + r0 * cols;
      for (int i = threadIdx.x; i < nt * cols; i += kThreads) {
        const int r = i / cols;
        sx[(i - r * cols) * kTile + r] = src[i];
      }
      __syncthreads();
    }
    for (int p = wv; p < P; p += kWaves) {
      int ca = pairs[2 * p], cb = pairs[2 * p + 1];
      if (!hx_guard((unsigned)ca < (unsigned)cols && (unsigned)cb < (unsigned)cols)) ca = cb = 0;
      double ma = 0.0, mb = 0.0;
      if (PASS == 2) {
        const long long n = counts[p * 4];
        ma = n > 0 ? sums[p * 5 + 0] / (double)n : 0.0;
        mb = n > 0 ? sums[p * 5 + 1] / (double)n : 0.0;
      }
      unsigned cn = 0, lt = 0, eq = 0, gt = 0;  // wave-uniform
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
      for (int j0 = 0; j0 < nt; j0 += 64) {
        const int j = j0 + lane;
        double a = nan, b = nan;
        if (j < nt) {
          a = staged ? sx[ca * kTile + j] : x[(r0 + j) * cols + ca];
          b = staged ? sx[cb * kTile + j] : x[(r0 + j) * cols + cb];
        }
        const bool v = a == a && b == b;
        if (PASS == 1) {
          cn += popc(v);
          lt += popc(v && a < b);
          eq += popc(v && a == b);
          gt += popc(v && a > b);
          s0 += v ? a : 0.0;
          s1 += v ? b : 0.0;
        } else {
          const double d = v ? a - ma : 0.0, e = v ? b - mb : 0.0;
          s0 += d;
          s1 += e;
          s2 += d * d;
          s3 += e * e;
          s4 += d * e;
        }
      }
      s0 = wave_sum_f64(s0);
      s1 = wave_sum_f64(s1);
      if (PASS == 2) {
        s2 = wave_sum_f64(s2);
        s3 = wave_sum_f64(s3);
        s4 = wave_sum_f64(s4);
      }
      if (lane == 0) {
        uint64_t* o = part + (long)p * kMomWords * ntiles + tile;
        if (PASS == 1) {
          o[0] = cn;
          o[ntiles] = lt;
          o[2 * ntiles] = eq;
          o[3 * ntiles] = gt;
          ((double*)o)[4 * ntiles] = s0;
          ((double*)o)[5 * ntiles] = s1;
        } else {
          ((double*)o)[0] = s0;
          ((double*)o)[ntiles] = s1;
          ((double*)o)[2 * ntiles] = s2;
          ((double*)o)[3 * ntiles] = s3;
          ((double*)o)[4 * ntiles] = s4;
        }
      }
    }
    __syncthreads();
  }
}

// one workgroup per pair: thread t adds tiles t, t + 256, ... in turn, then a fixed tree
template <int PASS>
__global__ __launch_bounds__(kThreads) void moments_sum_k(const uint64_t* __restrict__ part, int rows,
                                                          long long* __restrict__ counts, double* __restrict__ sums) {
  constexpr int kInts = PASS == 1 ? 4 : 0, kDbl = PASS == 1 ? 2 : 5;
  __shared__ unsigned long long si[4][kThreads];
  __shared__ double sd[5][kThreads];
  const int p = blockIdx.x, tid = threadIdx.x;
  const long ntiles = ((long)rows + kTile - 1) / kTile;
  const uint64_t* in = part + (long)p * kMomWords * ntiles;
  unsigned long long ai[4] = {0, 0, 0, 0};
  double ad[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (long t = tid; t < ntiles; t += kThreads) {
#pragma unroll
    for (int q = 0; q < kInts; ++q) ai[q] += in[q * ntiles + t];
#pragma unroll
    for (int q = 0; q < kDbl; ++q) ad[q] += ((const double*)in)[(kInts + q) * ntiles + t];
  }
#pragma unroll
  for (int q = 0; q < kInts; ++q) si[q][tid] = ai[q];
#pragma unroll
  for (int q = 0; q < kDbl; ++q) sd[q][tid] = ad[q];
  __syncthreads();
#pragma unroll
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int q = 0; q < kInts; ++q) si[q][tid] += si[q][tid + o];
#pragma unroll
      for (int q = 0; q < kDbl; ++q) sd[q][tid] += sd[q][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (PASS == 1) {
      for (int q = 0; q < 4; ++q) counts[p * 4 + q] = (long long)si[q][0];
      sums[p * 5 + 0] = sd[0][0];
      sums[p * 5 + 1] = sd[1][0];
    } else {
      const double n = (double)counts[p * 4];
      const double d = sd[0][0], e = sd[1][0];
      sums[p * 5 + 2] = n > 0.0 ? fmax(sd[2][0] - d * d / n, 0.0) : 0.0;
      sums[p * 5 + 3] = n > 0.0 ? fmax(sd[3][0] - e * e / n, 0.0) : 0.0;
      sums[p * 5 + 4] = n > 0.0 ? sd[4][0] - d * e / n : 0.0;
    }
  }
}

// ---- the distinct keys of a sorted column ----
// exclusive prefix of v over the workgroup's threads; *total = the sum.  Ends with a barrier.
__device__ __forceinline__ unsigned block_scan_u32(unsigned v, unsigned* wsum, unsigned* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  unsigned off = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    off += w < wv ? wsum[w] : 0u;
    all += wsum[w];
  }
  __syncthreads();
  *total = all;
  return off + inc - v;
}

// WRITE false: hc[c][tile] = run heads in the tile.  WRITE true (hc scanned): table[c][...] = the heads' keys, in order.
template <bool WRITE>
__global__ __launch_bounds__(kThreads) void heads_k(const uint64_t* __restrict__ keys, int rows,
                                                    unsigned* __restrict__ hc, uint64_t* __restrict__ table) {
  __shared__ unsigned wsum[kWaves];
  const int c = blockIdx.y, tid = threadIdx.x;
  const uint64_t* s = keys + (long)c * rows;
  const long ntiles = ((long)rows + kCTile - 1) / kCTile;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long j0 = tile * kCTile + (long)tid * kPerThread;
    uint64_t k[kPerThread];
    uint64_t prev = (j0 > 0 && j0 < rows) ? s[j0 - 1] : 0ull;
    unsigned head = 0, cnt = 0;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const long j = j0 + i;
      k[i] = j < rows ? s[j] : 0ull;
      const bool h = j < rows && (j == 0 || k[i] != prev);
      prev = k[i];
      head |= (unsigned)h << i;
      cnt += h;
    }
    unsigned total;
    unsigned pos = block_scan_u32(cnt, wsum, &total);
    if (!WRITE) {
      if (tid == 0) hc[(long)c * ntiles + tile] = total;
    } else {
      pos += hc[(long)c * ntiles + tile];
#pragma unroll
      for (int i = 0; i < kPerThread; ++i)
        if ((head >> i) & 1u) {
          if (hx_guard(pos < (unsigned)rows)) table[(long)c * rows + pos] = k[i];
          ++pos;
        }
    }
  }
}

// one workgroup per column: hc[c][tile] := heads in the earlier tiles, dcount[c] = all heads
__global__ __launch_bounds__(kThreads) void headscan_k(unsigned* __restrict__ hc, int rows,
                                                       long long* __restrict__ dcount) {
  __shared__ unsigned wsum[kWaves];
  const long ntiles = ((long)rows + kCTile - 1) / kCTile;
  unsigned* h = hc + (long)blockIdx.x * ntiles;
  unsigned running = 0;
  for (long t0 = 0; t0 < ntiles; t0 += kThreads) {
    const long i = t0 + threadIdx.x;
    unsigned total;
    const unsigned ex = block_scan_u32(i < ntiles ? h[i] : 0u, wsum, &total);
    if (i < ntiles) h[i] = running + ex;
    running += total;
  }
  if (threadIdx.x == 0) dcount[blockIdx.x] = running;
}

// index of k among the d distinct keys tab[0..d): lds holds the m samples tab[0], tab[s], tab[2 s], ...
__device__ __forceinline__ unsigned rank_of(const uint64_t* lds, int m, long s, const uint64_t* __restrict__ tab, long d,
                                            uint64_t k) {
  int lo = 0, hi = m;  // the first sample >= k
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (lds[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  long glo = lo == 0 ? 0 : (long)(lo - 1) * s + 1, ghi = lo == m ? d : (long)lo * s;  // empty when s == 1
  while (glo < ghi) {
    const long mid = glo + ((ghi - glo) >> 1);
    if (tab[mid] < k) glo = mid + 1;
    else ghi = mid;
  }
  return (unsigned)glo;
}

__global__ __launch_bounds__(kThreads) void rank_k(const double* __restrict__ x, int rows, int cols,
                                                   const int* __restrict__ pairs, const uint64_t* __restrict__ table,
                                                   const long long* __restrict__ dcount, uint64_t* __restrict__ comp) {
  __shared__ uint64_t ta[kTableKeys], tb[kTableKeys];
  const int p = blockIdx.y;
  int ca = pairs[2 * p], cb = pairs[2 * p + 1];
  if (!hx_guard((unsigned)ca < (unsigned)cols && (unsigned)cb < (unsigned)cols)) ca = cb = 0;
  const uint64_t* tab_a = table + (long)ca * rows;
  const uint64_t* tab_b = table + (long)cb * rows;
  long da = dcount[ca], db = dcount[cb];
  if (!hx_guard(da >= 1 && da <= rows && db >= 1 && db <= rows)) da = db = 1;
  const long sa = (da + kTableKeys - 1) / kTableKeys, sb = (db + kTableKeys - 1) / kTableKeys;
  const int ma = (int)((da + sa - 1) / sa), mb = (int)((db + sb - 1) / sb);
  for (int i = threadIdx.x; i < ma; i += kThreads) ta[i] = tab_a[i * sa];
  for (int i = threadIdx.x; i < mb; i += kThreads) tb[i] = tab_b[i * sb];
  __syncthreads();
  uint64_t* out = comp + (long)p * rows;
  for (long r = (long)blockIdx.x * kThreads + threadIdx.x; r < rows; r += (long)gridDim.x * kThreads) {
    const uint64_t ra = rank_of(ta, ma, sa, tab_a, da, key_of(x[r * cols + ca]));
    const uint64_t rb = rank_of(tb, mb, sb, tab_b, db, key_of(x[r * cols + cb]));
    out[r] = ra << 32 | rb;
  }
}

}  // namespace colpair

extern "C" int hopsx_column_pair_tile() { return colpair::kTile; }
extern "C" int hopsx_column_pair_table_keys() { return colpair::kTableKeys; }

extern "C" long hopsx_column_pair_part_words(long rows, int npairs) {
  if (rows < 0 || rows > 0x7fffffffl || npairs < 0) return -1;
  return (long)npairs * colpair::kMomWords * colpair::tiles_of(rows, colpair::kTile);
}

extern "C" long hopsx_column_pair_head_words(long rows, int cols) {
  if (rows < 0 || rows > 0x7fffffffl || cols < 0) return -1;
  return (long)cols * colpair::tiles_of(rows, colpair::kCTile);
}

extern "C" int hopsx_column_pair_moments64(const double* x, long rows, int cols, const int* pairs, int npairs,
                                           unsigned long long* part, long long* counts, double* sums,
                                           int max_workgroups, hipStream_t st) {
  using namespace colpair;
  if (rows < 0 || rows > 0x7fffffffl || cols < 0 || npairs < 0 || max_workgroups < 0) return (int)hipErrorInvalidValue;
  if (rows == 0 || npairs == 0) return (int)hipSuccess;
  if (cols == 0 || !x || !pairs || !part || !counts || !sums) return (int)hipErrorInvalidValue;
  const int R = (int)rows;
  const dim3 grid(grid_x(tiles_of(rows, kTile), 1, max_workgroups)), block(kThreads);
  uint64_t* pw = (uint64_t*)part;
  hipLaunchKernelGGL(moments_k<1>, grid, block, 0, st, x, R, cols, pairs, npairs, (const long long*)counts,
                     (const double*)sums, pw);
  hipLaunchKernelGGL(moments_sum_k<1>, dim3(npairs), block, 0, st, (const uint64_t*)pw, R, counts, sums);
  hipLaunchKernelGGL(moments_k<2>, grid, block, 0, st, x, R, cols, pairs, npairs, (const long long*)counts,
                     (const double*)sums, pw);
  hipLaunchKernelGGL(moments_sum_k<2>, dim3(npairs), block, 0, st, (const uint64_t*)pw, R, counts, sums);
  return (int)hipGetLastError();
}

extern "C" int hopsx_column_pair_ranks64(const double* x, long rows, int cols, const int* pairs, int npairs,
                                         const unsigned long long* sorted, unsigned long long* table, unsigned* heads,
                                         long long* dcount, unsigned long long* comp, int max_workgroups,
                                         hipStream_t st) {
  using namespace colpair;
  if (rows < 0 || rows > 0x7fffffffl || cols < 0 || npairs < 0 || max_workgroups < 0) return (int)hipErrorInvalidValue;
  if (rows == 0 || cols == 0) return (int)hipSuccess;
  if (!x || !sorted || !table || !heads || !dcount || (npairs > 0 && (!pairs || !comp))) return (int)hipErrorInvalidValue;
  const int R = (int)rows;
  const dim3 block(kThreads), cgrid(grid_x(tiles_of(rows, kCTile), cols, max_workgroups), cols);
  hipLaunchKernelGGL(heads_k<false>, cgrid, block, 0, st, (const uint64_t*)sorted, R, heads, (uint64_t*)table);
  hipLaunchKernelGGL(headscan_k, dim3(cols), block, 0, st, heads, R, dcount);
  hipLaunchKernelGGL(heads_k<true>, cgrid, block, 0, st, (const uint64_t*)sorted, R, heads, (uint64_t*)table);
  if (npairs > 0)
    hipLaunchKernelGGL(rank_k, dim3(grid_x(tiles_of(rows, kThreads), npairs, max_workgroups), npairs), block, 0, st, x,
                       R, cols, pairs, (const uint64_t*)table, (const long long*)dcount, (uint64_t*)comp);
  return (int)hipGetLastError();
}

HOPSX_DBG_TU(colpair)
