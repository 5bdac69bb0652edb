// hopsx: equi-joins of fp64 feature frames over sorted stacked keys (gfx950): what `a JOIN b ON a.k = b.k` (inner, left,
// full) returns as row index pairs, and the gather of the joined columns.  NaN is NULL: a NaN key matches nothing.
//
// Input: the key columns of the left frame stacked over those of the right one, turned into code << 32 | row
// (hopsx_group_keys64) and sorted (hopsx_column_sort_keys64), n = nl + nr keys.  A run of one code holds its left rows
// (row < nl) ascending, then its right rows ascending; the rows with a NaN key are the tail.  Everything below is
// integers and copied bits, so every result is exact and independent of the grid.
//
//   hopsx_join_spans64    the runs (hopsx_group_heads64: seg_off, G), split[g] = the run's first right position, one
//                         binary search per RUN (split_k, a thread per run), then spans_k: a workgroup per tile of
//                         kTile sorted positions finds each position's run as group_reduce_k does (the tile's first run
//                         by one search, then a popcount over the head ballots kept in LDS) and writes, per left row,
//                         rbeg / rcnt (its run's right rows) and, per right row, lcnt (its run's left rows).
//   hopsx_join_offsets64  the exclusive 64-bit scan of f(cnt[i]) in row order, f = cnt (inner), max(cnt, 1) (left,
//                         full) or cnt == 0 (the flags of the full join's tail): totals_k per tile of kTile rows,
//                         scantot_k (one workgroup) over the tile totals, local_k inside every tile.  Three launches,
//                         no workgroup ever waits for another.  info = the total and the rows with cnt > 0.
//   hopsx_join_expand64   a workgroup owns kTile OUTPUT positions [t0, t1): two binary searches in the global offsets
//                         give the left rows lf..ll that cover them; their offsets go to LDS in chunks of kTableRows
//                         (+ 1: the chunk's end), and every lane searches the chunk for each of its positions t that
//                         lies inside it: l = the last row with off[l] <= t, j = t - off[l], li[t] = l, ri[t] = the
//                         row behind keys[rbeg[l] + j] (-1: a left row without a match).  One row with a million
//                         matches spreads over a thousand workgroups; rows without output are skipped by the searches.
//   hopsx_join_tail64     local_k with the scatter: the right rows with lcnt == 0, in row order, behind the main part.
//   hopsx_join_gather64   out[t][c] from xl[li[t]][cols[c]] / xr[ri[t]][cols[c]], NaN for -1: a workgroup stages the
//                         indices of kGatherRows output rows in LDS and its lanes run over the flat (t, c) index, so a
//                         wave stores 512 consecutive bytes and no index is loaded twice from memory.
#include "common.h"
#include "ops_api.h"

namespace hjoin {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / HOPSX_WAVE;
constexpr int kTile = 1024;  // output positions (expand), sorted positions (spans), rows (scan) per tile
constexpr int kChunks = kTile / HOPSX_WAVE;
constexpr int kWaveChunks = kChunks / kWaves;
constexpr int kPerThread = kTile / kThreads;
constexpr int kTableRows = 1024;  // offsets an LDS chunk of expand_k holds (8 KiB)
constexpr int kGatherRows = 256;  // output rows whose indices gather_k stages
constexpr unsigned kDropCode = 0xFFFFFFFFu;
constexpr int kDefaultGrid = 4096;

static inline long tiles_of(long rows, int tile = kTile) { return (rows + tile - 1) / tile; }
static inline int grid_x(long n, int max_workgroups) {
  long gx = max_workgroups > 0 ? max_workgroups : kDefaultGrid;
  if (gx > n) gx = n;
  return (int)(gx < 1 ? 1 : gx);
}

// ---- spans ----
// split[g] = the first position of run g whose row is a right row (seg_off[g + 1]: none)
__global__ __launch_bounds__(kThreads) void join_split_k(const uint64_t* __restrict__ keys, long n, unsigned nl,
                                                         const long long* __restrict__ seg_off,
                                                         const long long* __restrict__ ginfo,
                                                         long long* __restrict__ split) {
  long G = ginfo[0];
  if (!hx_guard(G >= 0 && G <= n)) G = 0;
  for (long g = (long)blockIdx.x * kThreads + threadIdx.x; g < G; g += (long)gridDim.x * kThreads) {
    long lo = seg_off[g], hi = seg_off[g + 1];
    if (!hx_guard(lo >= 0 && lo <= hi && hi <= n)) lo = hi = 0;
    while (lo < hi) {
      const long mid = lo + ((hi - lo) >> 1);
      if ((unsigned)keys[mid] < nl) lo = mid + 1;
      else hi = mid;
    }
    split[g] = lo;
  }
}

// heads at the tile positions [0, j]
__device__ __forceinline__ int heads_upto(const uint64_t* sball, int j) {
  int h = 0;
  for (int k = 0; k < (j >> 6); ++k) h += __popcll(sball[k]);
  return h + __popcll(sball[j >> 6] & (~0ull >> (63 - (j & 63))));
}

__global__ __launch_bounds__(kThreads) void join_spans_k(const uint64_t* __restrict__ keys, long n, unsigned nl,
                                                         unsigned nr, const long long* __restrict__ seg_off,
                                                         const long long* __restrict__ ginfo,
                                                         const long long* __restrict__ split, int* __restrict__ rbeg,
                                                         unsigned* __restrict__ rcnt, unsigned* __restrict__ lcnt) {
  __shared__ uint64_t sball[kChunks];
  __shared__ long long sg0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  long G = ginfo[0], nvalid = ginfo[1];  // the runs, the positions in a run (behind them: the NaN keys)
  if (!hx_guard(G >= 0 && G <= n && nvalid >= 0 && nvalid <= n && (G > 0) == (nvalid > 0))) G = nvalid = 0;
  const long ntiles = (n + kTile - 1) / kTile;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long p0 = tile * kTile;
    const int nt = (int)(nvalid - p0 < kTile ? (nvalid - p0 > 0 ? nvalid - p0 : 0) : kTile);
    uint64_t kk[kWaveChunks];
#pragma unroll
    for (int q = 0; q < kWaveChunks; ++q) {
      const int k = wv * kWaveChunks + q, j = k * 64 + lane;
      const long p = p0 + j;
      const bool in = j < nt;
      kk[q] = p < n ? keys[p] : 0ull;
      const uint64_t prev = (in && p > 0) ? keys[p - 1] : 0ull;
      const uint64_t b = __ballot(in && (p == 0 || (kk[q] >> 32) != (prev >> 32)));
      if (lane == 0) sball[k] = b;
    }
    if (threadIdx.x == 0) {
      long lo = 0, hi = G;  // the run of p0: the last g with seg_off[g] <= p0
      while (hi - lo > 1) {
        const long mid = lo + ((hi - lo) >> 1);
        if (seg_off[mid] <= p0) lo = mid;
        else hi = mid;
      }
      sg0 = lo;
    }
    __syncthreads();
    const long long gbase = sg0 - (long long)(sball[0] & 1ull);  // run of j = gbase + heads_upto(j)
#pragma unroll
    for (int q = 0; q < kWaveChunks; ++q) {
      const int j = (wv * kWaveChunks + q) * 64 + lane;
      const long p = p0 + j;
      if (p >= n) continue;
      long long a = 0, s = 0, b = 0;
      if (j < nt) {
        const long long g = gbase + heads_upto(sball, j);
        if (hx_guard(g >= 0 && g < G)) {
          a = seg_off[g], s = split[g], b = seg_off[g + 1];
          if (!hx_guard(a <= p && p < b && a <= s && s <= b && b <= nvalid)) a = s = b = 0;
        }
      }
      const unsigned row = (unsigned)kk[q];
      if (row < nl) {
        rbeg[row] = (int)s;
        rcnt[row] = (unsigned)(b - s);
      } else if (hx_guard(row - nl < nr)) {
        lcnt[row - nl] = (unsigned)(s - a);
      }
    }
    __syncthreads();  // sball and sg0 are free for the next tile
  }
}

// ---- offsets ----
// what a row adds to the scan: MODE 0 its count, 1 at least one (an unmatched left row is kept), 2 the flag count == 0
template <int MODE>
__device__ __forceinline__ unsigned scan_val(unsigned v) {
  return MODE == 0 ? v : MODE == 1 ? (v > 1u ? v : 1u) : (v == 0u ? 1u : 0u);
}

// exclusive prefix of v over the workgroup's threads; *total = the sum.  Ends with a barrier.
__device__ __forceinline__ unsigned long long block_scan_u64(unsigned long long v, unsigned long long* wsum,
                                                             unsigned long long* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned long long inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  unsigned long long off = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    off += w < wv ? wsum[w] : 0ull;
    all += wsum[w];
  }
  __syncthreads();
  *total = all;
  return off + inc - v;
}

// tot[tile] = the sum of f over the tile's rows, nz[tile] = its rows with a count
template <int MODE>
__global__ __launch_bounds__(kThreads) void join_totals_k(const unsigned* __restrict__ cnt, long m,
                                                          unsigned long long* __restrict__ tot,
                                                          unsigned* __restrict__ nz) {
  __shared__ unsigned long long wsum[kWaves];
  const long ntiles = (m + kTile - 1) / kTile;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long i0 = tile * kTile + (long)threadIdx.x * kPerThread;
    unsigned long long s = 0, z = 0;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i)
      if (i0 + i < m) {
        const unsigned v = cnt[i0 + i];
        s += scan_val<MODE>(v);
        z += v != 0u;
      }
    unsigned long long ts, tz;
    block_scan_u64(s, wsum, &ts);
    block_scan_u64(z, wsum, &tz);
    if (threadIdx.x == 0) {
      tot[tile] = ts;
      nz[tile] = (unsigned)tz;
    }
  }
}

// one workgroup: tot[tile] := the sum of the earlier tiles; info = the total, the rows with a count; off_end = total
__global__ __launch_bounds__(kThreads) void join_scantot_k(unsigned long long* __restrict__ tot,
                                                           const unsigned* __restrict__ nz, long ntiles,
                                                           long long* __restrict__ info,
                                                           long long* __restrict__ off_end) {
  __shared__ unsigned long long wsum[kWaves];
  unsigned long long running = 0, matched = 0;
  for (long t0 = 0; t0 < ntiles; t0 += kThreads) {
    const long i = t0 + threadIdx.x;
    unsigned long long total, tz;
    const unsigned long long ex = block_scan_u64(i < ntiles ? tot[i] : 0ull, wsum, &total);
    block_scan_u64(i < ntiles ? (unsigned long long)nz[i] : 0ull, wsum, &tz);
    if (i < ntiles) tot[i] = running + ex;
    running += total;
    matched += tz;
  }
  if (threadIdx.x == 0) {
    info[0] = (long long)running;
    info[1] = (long long)matched;
    if (off_end) *off_end = (long long)running;
  }
}

// SCATTER false: off[i] = the scan.  SCATTER true (MODE 2): the flagged rows go to li / ri [base + scan] as (-1, row).
template <int MODE, bool SCATTER>
__global__ __launch_bounds__(kThreads) void join_local_k(const unsigned* __restrict__ cnt, long m,
                                                         const unsigned long long* __restrict__ tot,
                                                         long long* __restrict__ off, long base, long n_out,
                                                         int* __restrict__ li, int* __restrict__ ri) {
  __shared__ unsigned long long wsum[kWaves];
  const long ntiles = (m + kTile - 1) / kTile;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long i0 = tile * kTile + (long)threadIdx.x * kPerThread;
    unsigned v[kPerThread];
    unsigned long long s = 0;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      v[i] = i0 + i < m ? scan_val<MODE>(cnt[i0 + i]) : 0u;
      s += v[i];
    }
    unsigned long long total;
    unsigned long long pos = tot[tile] + block_scan_u64(s, wsum, &total);
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      if (i0 + i >= m) break;
      if (!SCATTER) {
        off[i0 + i] = (long long)pos;
      } else if (v[i]) {
        const long t = base + (long)pos;
        if (hx_guard(t >= base && t < n_out)) {
          li[t] = -1;
          ri[t] = (int)(i0 + i);
        }
      }
      pos += v[i];
    }
  }
}

// ---- balanced expand ----
__global__ __launch_bounds__(kThreads) void join_expand_k(const uint64_t* __restrict__ keys, long n, long nl, long nr,
                                                          const long long* __restrict__ off,
                                                          const int* __restrict__ rbeg,
                                                          const unsigned* __restrict__ rcnt, long n_main,
                                                          int* __restrict__ li, int* __restrict__ ri) {
  __shared__ long long soff[kTableRows + 1];
  __shared__ long sl[2];
  const long ntiles = (n_main + kTile - 1) / kTile;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long t0 = tile * kTile;
    const long t1 = t0 + kTile < n_main ? t0 + kTile : n_main;
    if (threadIdx.x < 2) {  // the last left row with off[l] <= t0 resp. t1 - 1: it has output there (off[l + 1] is larger)
      const long target = threadIdx.x == 0 ? t0 : t1 - 1;
      long lo = 0, hi = nl;
      while (hi - lo > 1) {
        const long mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= target) lo = mid;
        else hi = mid;
      }
      sl[threadIdx.x] = lo;
    }
    __syncthreads();
    const long lf = sl[0], ll = sl[1];
    for (long lc = lf; lc <= ll; lc += kTableRows) {  // workgroup-uniform
      const int nc = (int)(ll - lc + 1 < kTableRows ? ll - lc + 1 : kTableRows);
      for (int i = threadIdx.x; i <= nc; i += kThreads) soff[i] = off[lc + i];  // lc + nc <= nl: off holds nl + 1
      __syncthreads();
      const long long c0 = soff[0], c1 = soff[nc];  // this chunk's rows cover [c0, c1); the first chunk's c0 <= t0
#pragma unroll
      for (int i = 0; i < kPerThread; ++i) {
        const long t = t0 + i * kThreads + threadIdx.x;
        if (t >= t1 || t < c0 || t >= c1) continue;
        int lo = 0, hi = nc;  // the last row of the chunk with soff <= t
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (soff[mid] <= t) lo = mid;
          else hi = mid;
        }
        const long l = lc + lo;
        const long j = t - soff[lo];
        const unsigned rc = rcnt[l];
        int r = -1;
        if (rc != 0u && hx_guard(j >= 0 && j < (long)rc)) {
          const long pos = (long)rbeg[l] + j;
          if (hx_guard(pos >= 0 && pos < n)) {
            const long row = (long)(unsigned)keys[pos] - nl;
            if (hx_guard(row >= 0 && row < nr)) r = (int)row;
          }
        }
        li[t] = (int)l;
        ri[t] = r;
      }
      __syncthreads();  // soff is free for the next chunk; sl for the next tile
    }
  }
}

// ---- gather ----
__global__ __launch_bounds__(kThreads) void join_gather_k(const double* __restrict__ xl, long nl, int colsl,
                                                          const double* __restrict__ xr, long nr, int colsr,
                                                          const int* __restrict__ li, const int* __restrict__ ri,
                                                          long n_out, const int* __restrict__ cols, int CL, int CR,
                                                          double* __restrict__ out) {
  __shared__ int sli[kGatherRows], sri[kGatherRows];
  const int C = CL + CR;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const long ntiles = (n_out + kGatherRows - 1) / kGatherRows;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long t0 = tile * kGatherRows;
    const int nt = (int)(n_out - t0 < kGatherRows ? n_out - t0 : kGatherRows);
    if ((int)threadIdx.x < nt) {
      int a = li[t0 + threadIdx.x], b = ri[t0 + threadIdx.x];
      if (!hx_guard(a >= -1 && a < nl)) a = -1;
      if (!hx_guard(b >= -1 && b < nr)) b = -1;
      sli[threadIdx.x] = a;
      sri[threadIdx.x] = b;
    }
    __syncthreads();
    const long total = (long)nt * C;
    for (long i = threadIdx.x; i < total; i += kThreads) {
      const int t = (int)(i / C), c = (int)(i - (long)t * C);
      const int col = cols[c];
      double v = nan;
      if (c < CL) {
        const int a = sli[t];
        if (a >= 0 && hx_guard(col >= 0 && col < colsl)) v = xl[(long)a * colsl + col];
      } else {
        const int b = sri[t];
        if (b >= 0 && hx_guard(col >= 0 && col < colsr)) v = xr[(long)b * colsr + col];
      }
      out[t0 * C + i] = v;
    }
    __syncthreads();
  }
}

template <int MODE>
static void launch_totals(const unsigned* cnt, long m, unsigned long long* tot, unsigned* nz, long long* off,
                          long long* info, int max_workgroups, hipStream_t st) {
  const long ntiles = tiles_of(m);
  const dim3 grid(grid_x(ntiles, max_workgroups)), block(kThreads);
  hipLaunchKernelGGL(join_totals_k<MODE>, grid, block, 0, st, cnt, m, tot, nz);
  hipLaunchKernelGGL(join_scantot_k, dim3(1), block, 0, st, tot, (const unsigned*)nz, ntiles, info,
                     off ? off + m : (long long*)nullptr);
  if (off)
    hipLaunchKernelGGL((join_local_k<MODE, false>), grid, block, 0, st, cnt, m, (const unsigned long long*)tot, off, 0l,
                       0l, (int*)nullptr, (int*)nullptr);
}

}  // namespace hjoin

extern "C" int hopsx_join_tile() { return hjoin::kTile; }
extern "C" int hopsx_join_table_rows() { return hjoin::kTableRows; }

extern "C" int hopsx_join_spans64(const unsigned long long* keys, long nl, long nr, unsigned* heads, long long* seg_off,
                                  long long* first_row, long long* ginfo, long long* split, int* rbeg, unsigned* rcnt,
                                  unsigned* lcnt, int max_workgroups, hipStream_t st) {
  using namespace hjoin;
  if (nl < 1 || nr < 1 || nl + nr > 0x7fffffffl || max_workgroups < 0 || !keys || !heads || !seg_off || !first_row ||
      !ginfo || !split || !rbeg || !rcnt || !lcnt)
    return (int)hipErrorInvalidValue;
  const long n = nl + nr;
  const int e = hopsx_group_heads64(keys, n, heads, seg_off, first_row, ginfo, max_workgroups, st);
  if (e) return e;
  const dim3 block(kThreads);
  hipLaunchKernelGGL(join_split_k, dim3(grid_x(tiles_of(n, kThreads), max_workgroups)), block, 0, st,
                     (const uint64_t*)keys, n, (unsigned)nl, (const long long*)seg_off, (const long long*)ginfo, split);
  hipLaunchKernelGGL(join_spans_k, dim3(grid_x(tiles_of(n), max_workgroups)), block, 0, st, (const uint64_t*)keys, n,
                     (unsigned)nl, (unsigned)nr, (const long long*)seg_off, (const long long*)ginfo,
                     (const long long*)split, rbeg, rcnt, lcnt);
  return (int)hipGetLastError();
}

extern "C" int hopsx_join_offsets64(const unsigned* cnt, long m, int mode, unsigned long long* tot, unsigned* nz,
                                    long long* off, long long* info, int max_workgroups, hipStream_t st) {
  using namespace hjoin;
  if (m < 1 || m > 0x7fffffffl || mode < 0 || mode > 2 || max_workgroups < 0 || !cnt || !tot || !nz || !info)
    return (int)hipErrorInvalidValue;
  if (mode == 0) launch_totals<0>(cnt, m, tot, nz, off, info, max_workgroups, st);
  else if (mode == 1) launch_totals<1>(cnt, m, tot, nz, off, info, max_workgroups, st);
  else launch_totals<2>(cnt, m, tot, nz, off, info, max_workgroups, st);
  return (int)hipGetLastError();
}

extern "C" int hopsx_join_expand64(const unsigned long long* keys, long nl, long nr, const long long* off,
                                   const int* rbeg, const unsigned* rcnt, long n_main, int* li, int* ri,
                                   int max_workgroups, hipStream_t st) {
  using namespace hjoin;
  if (nl < 1 || nr < 1 || nl + nr > 0x7fffffffl || n_main < 0 || n_main > 0x7fffffffl || max_workgroups < 0)
    return (int)hipErrorInvalidValue;
  if (n_main == 0) return (int)hipSuccess;
  if (!keys || !off || !rbeg || !rcnt || !li || !ri) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(join_expand_k, dim3(grid_x(tiles_of(n_main), max_workgroups)), dim3(kThreads), 0, st,
                     (const uint64_t*)keys, nl + nr, nl, nr, off, rbeg, rcnt, n_main, li, ri);
  return (int)hipGetLastError();
}

extern "C" int hopsx_join_tail64(const unsigned* lcnt, long nr, const unsigned long long* tot, long base, long n_out,
                                 int* li, int* ri, int max_workgroups, hipStream_t st) {
  using namespace hjoin;
  if (nr < 1 || nr > 0x7fffffffl || base < 0 || n_out < base || n_out > 0x7fffffffl || max_workgroups < 0)
    return (int)hipErrorInvalidValue;
  if (n_out == base) return (int)hipSuccess;
  if (!lcnt || !tot || !li || !ri) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((join_local_k<2, true>), dim3(grid_x(tiles_of(nr), max_workgroups)), dim3(kThreads), 0, st, lcnt,
                     nr, tot, (long long*)nullptr, base, n_out, li, ri);
  return (int)hipGetLastError();
}

extern "C" int hopsx_join_gather64(const double* xl, long nl, int colsl, const double* xr, long nr, int colsr,
                                   const int* li, const int* ri, long n_out, const int* cols, int CL, int CR,
                                   double* out, int max_workgroups, hipStream_t st) {
  using namespace hjoin;
  if (nl < 0 || nr < 0 || nl > 0x7fffffffl || nr > 0x7fffffffl || colsl < 0 || colsr < 0 || n_out < 0 ||
      n_out > 0x7fffffffl || CL < 0 || CR < 0 || CL > 0xffff || CR > 0xffff || max_workgroups < 0)
    return (int)hipErrorInvalidValue;
  if (n_out == 0 || CL + CR == 0) return (int)hipSuccess;
  if (!li || !ri || !cols || !out || (CL && nl && !xl) || (CR && nr && !xr)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(join_gather_k, dim3(grid_x(tiles_of(n_out, kGatherRows), max_workgroups)), dim3(kThreads), 0, st, xl,
                     nl, colsl, xr, nr, colsr, li, ri, n_out, cols, CL, CR, out);
  return (int)hipGetLastError();
}

HOPSX_DBG_TU(join)
