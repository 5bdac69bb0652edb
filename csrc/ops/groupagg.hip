// hopsx: group-by aggregates of fp64 feature columns (gfx950): count, sum, min, max, mean and the sample variance of
// V value columns per group of 1..4 key columns, what pandas' groupby(by, sort=True)[values].agg(...) and Spark's
// groupBy().agg() return.  NaN is missing: a row with a NaN key belongs to no group, a NaN value is skipped.
//
//   hopsx_group_keys64    key[row] = code << 32 | row, code the mixed-radix number of the row's dense ranks in the key
//                         columns (hopsx_column_pair_ranks64's low words), the first key most significant; a row with
//                         a NaN key gets code 0xFFFFFFFF.  Sorted by hopsx_column_sort_keys64 the groups are runs of
//                         one code in pandas' order, the rows of a run ascending, the dropped rows the tail.
//   hopsx_group_heads64   seg_off[G + 1] = where every run starts (seg_off[G] = the rows that are in a group),
//                         first_row[G] = the row of the run's head, info = G and seg_off[G].
//   hopsx_group_reduce64  out[g][c] over the rows of group g, every sum in an order fixed by kTile alone.
//
// Reduce: a workgroup owns a tile of kTile sorted positions, wave w its span of 256.  The lanes split their keys into
// code and row; the head flags go to LDS as one ballot per 64 positions (the group of a position is the tile's first
// group plus a popcount).  Per block of kColBlock columns the rows' values are gathered into LDS, consecutive lanes
// reading the consecutive doubles of one row, and written transposed.  Per column a wave runs a segmented inclusive
// scan over its four ballots (shuffles, a lane stops at its run's head; the carry between the four is the last lane's)
// and writes every run that starts inside its span.  The run that enters a span from the left is finished after a
// barrier by one thread per column and wave: the tails of the earlier waves back to the last one with a head, added in
// wave order, then the span's own lead.  A run that starts and ends inside the tile goes straight to out[g]; the run
// open to the left goes to the tile's partial 0, the one open to the right to partial 1 (a run over the whole tile is
// partial 0 alone).  finish_k: a wave per tile whose partial 1 is set owns that group, its lanes add the group's
// partials round-robin in tile order, then a fixed butterfly.  No float atomics, and a partial depends on its tile
// alone, so the bits do not depend on the grid.
//
// The second pass (var) is the same kernel on d = x - mean[g]: sum d and sum d^2, M2 = sum d^2 - (sum d)^2 / n
// (clamped at 0), var = M2 / (n - 1), NaN for n < 2.
#include "common.h"
#include "ops_api.h"

namespace groupagg {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / HOPSX_WAVE;
constexpr int kTile = 1024;                   // sorted positions per tile
constexpr int kChunks = kTile / HOPSX_WAVE;   // ballots per tile
constexpr int kWaveChunks = kChunks / kWaves;
constexpr int kSpan = kTile / kWaves;         // positions per wave
constexpr int kPerThread = kTile / kThreads;  // positions per thread of heads_k
// LDS of reduce_k: kColBlock x kTile doubles staged (48 KiB) + the rows (4 KiB) + leads and tails (2 KiB) under 64 KiB
constexpr int kColBlock = 6;
constexpr int kMaxKeys = 4;
constexpr unsigned kDropCode = 0xFFFFFFFFu;
constexpr int kDefaultGrid = 4096;

static inline long tiles_of(long rows) { return (rows + kTile - 1) / kTile; }
static inline int grid_x(long n, int max_workgroups) {
  long gx = max_workgroups > 0 ? max_workgroups : kDefaultGrid;
  if (gx > n) gx = n;
  return (int)(gx < 1 ? 1 : gx);
}

struct KeyPlan {
  int col[kMaxKeys];
  unsigned radix[kMaxKeys], mult[kMaxKeys];
};

// comp: [nkeys][rows], the low word of comp[k][r] = the rank of x[r][col[k]] among its column's classes
__global__ __launch_bounds__(kThreads) void group_keys_k(const double* __restrict__ x, int rows, int cols, int nkeys,
                                                         KeyPlan plan, const uint64_t* __restrict__ comp,
                                                         uint64_t* __restrict__ keys) {
  for (long r = (long)blockIdx.x * kThreads + threadIdx.x; r < rows; r += (long)gridDim.x * kThreads) {
    uint64_t code = 0;
    bool drop = false;
    for (int k = 0; k < nkeys; ++k) {
      const double v = x[r * cols + plan.col[k]];
      unsigned rank = (unsigned)comp[(long)k * rows + r];
      if (!hx_guard(rank < plan.radix[k])) rank = 0;
      drop |= v != v;
      code += (uint64_t)rank * plan.mult[k];
    }
    keys[r] = (drop ? (uint64_t)kDropCode : code) << 32 | (uint64_t)r;
  }
}

// ---- the runs of the sorted keys ----
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

// WRITE false: hc[tile] = the heads in the tile.  WRITE true (hc scanned, info[0] = G): seg_off, first_row, info[1].
template <bool WRITE>
__global__ __launch_bounds__(kThreads) void group_heads_k(const uint64_t* __restrict__ keys, int rows,
                                                          unsigned* __restrict__ hc, long long* __restrict__ seg_off,
                                                          long long* __restrict__ first_row,
                                                          long long* __restrict__ info) {
  __shared__ unsigned wsum[kWaves];
  const long ntiles = ((long)rows + kTile - 1) / kTile;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long j0 = tile * kTile + (long)threadIdx.x * kPerThread;
    uint64_t k[kPerThread];
    unsigned prev = (j0 > 0 && j0 < rows) ? (unsigned)(keys[j0 - 1] >> 32) : 0u;
    unsigned head = 0, cnt = 0;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const long j = j0 + i;
      k[i] = j < rows ? keys[j] : ~0ull;
      const unsigned code = (unsigned)(k[i] >> 32);
      const bool h = j < rows && code != kDropCode && (j == 0 || code != prev);
      if (WRITE && j < rows) {  // the end of the grouped rows: the first dropped key, or the end of the keys
        long long* end = seg_off + info[0];
        if (code == kDropCode && (j == 0 || prev != kDropCode)) *end = info[1] = j;
        if (code != kDropCode && j == rows - 1) *end = info[1] = rows;
      }
      prev = code;
      head |= (unsigned)h << i;
      cnt += h;
    }
    unsigned total;
    unsigned pos = block_scan_u32(cnt, wsum, &total);
    if (!WRITE) {
      if (threadIdx.x == 0) hc[tile] = total;
    } else {
      pos += hc[tile];
#pragma unroll
      for (int i = 0; i < kPerThread; ++i)
        if ((head >> i) & 1u) {
          if (hx_guard(pos < (unsigned)rows)) {
            seg_off[pos] = j0 + i;
            first_row[pos] = (long long)(unsigned)k[i];
          }
          ++pos;
        }
    }
  }
}

// one workgroup: hc[tile] := the heads in the earlier tiles, info[0] = all heads
__global__ __launch_bounds__(kThreads) void group_headscan_k(unsigned* __restrict__ hc, int rows,
                                                             long long* __restrict__ info) {
  __shared__ unsigned wsum[kWaves];
  const long ntiles = ((long)rows + kTile - 1) / kTile;
  unsigned running = 0;
  for (long t0 = 0; t0 < ntiles; t0 += kThreads) {
    const long i = t0 + threadIdx.x;
    unsigned total;
    const unsigned ex = block_scan_u32(i < ntiles ? hc[i] : 0u, wsum, &total);
    if (i < ntiles) hc[i] = running + ex;
    running += total;
  }
  if (threadIdx.x == 0) info[0] = running;
}

// ---- the segmented reduction ----
// PASS 1: n, sum, min, max of the non-NaN values, the sum as an unevaluated pair hi + lo: every addition of two sums
// keeps its rounding error (Knuth's two-sum) in lo, so a group whose values cancel comes out as close to the exact sum
// as the compensated sum of the pandas route does, still in an order fixed by the positions.  PASS 2: sum d, sum d^2
// with d = x - mean[g], plain: the squares do not cancel.
constexpr int kPartWords = 5;
template <int PASS>
struct Acc {
  static constexpr int N = PASS == 1 ? kPartWords : 2;  // PASS 1: n, hi, lo, min, max
  double v[N];
};
template <int PASS>
__device__ __forceinline__ Acc<PASS> acc_none() {
  Acc<PASS> a;
  a.v[0] = a.v[1] = 0.0;
  if constexpr (PASS == 1) {
    a.v[2] = 0.0;
    a.v[3] = __longlong_as_double(0x7ff0000000000000ll);
    a.v[4] = -a.v[3];
  }
  return a;
}
// left (the earlier positions) first
template <int PASS>
__device__ __forceinline__ Acc<PASS> comb(const Acc<PASS>& l, const Acc<PASS>& r) {
  Acc<PASS> a;
  a.v[0] = l.v[0] + r.v[0];
  a.v[1] = l.v[1] + r.v[1];
  if constexpr (PASS == 1) {
    const double bb = a.v[1] - l.v[1];
    a.v[2] = (l.v[2] + r.v[2]) + ((l.v[1] - (a.v[1] - bb)) + (r.v[1] - bb));
    a.v[3] = fmin(l.v[3], r.v[3]);
    a.v[4] = fmax(l.v[4], r.v[4]);
  }
  return a;
}

struct Out {
  long long* count;
  double *sum, *mn, *mx, *mean, *var;
};

// part: hdr int64 [ntiles][2] (the group of the tile's partial, -1 none), then fp64 [ntiles][2][V][kPartWords]
__device__ __forceinline__ long long* part_hdr(uint64_t* part, long tile) { return (long long*)part + tile * 2; }
__device__ __forceinline__ double* part_val(uint64_t* part, long ntiles, long tile, int slot, int V, int c) {
  return (double*)part + ntiles * 2 + ((tile * 2 + slot) * V + c) * kPartWords;
}

template <int PASS>
__device__ __forceinline__ void write_group(const Acc<PASS>& a, long long g, long G, int V, int c, const Out& o) {
  if (!hx_guard(g >= 0 && g < G)) return;
  const long i = g * V + c;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if constexpr (PASS == 1) {
    const double n = a.v[0];
    const double s = isinf(a.v[1]) ? a.v[1] : a.v[1] + a.v[2];  // (an infinite sum has no error term)
    o.count[i] = (long long)n;
    o.sum[i] = s;
    o.mn[i] = n > 0.0 ? a.v[3] : nan;
    o.mx[i] = n > 0.0 ? a.v[4] : nan;
    o.mean[i] = n > 0.0 ? s / n : nan;
  } else {
    const double n = (double)o.count[i];
    o.var[i] = n > 1.0 ? fmax(a.v[1] - a.v[0] * a.v[0] / n, 0.0) / (n - 1.0) : nan;
  }
}

// a finished run of the tile: inside -> out[g]; open to the left -> partial 0; open to the right only -> partial 1
template <int PASS>
__device__ __forceinline__ void emit(const Acc<PASS>& a, bool starts_here, bool ends_here, long long g, long G, int V,
                                     int c, const Out& o, uint64_t* part, long ntiles, long tile) {
  if (starts_here && ends_here) {
    write_group<PASS>(a, g, G, V, c, o);
    return;
  }
  double* p = part_val(part, ntiles, tile, starts_here ? 1 : 0, V, c);
#pragma unroll
  for (int q = 0; q < Acc<PASS>::N; ++q) p[q] = a.v[q];
}

// the head flag of tile position j (j == nt: of the position behind the tile's last one)
__device__ __forceinline__ bool head_at(const uint64_t* sball, int j) { return (sball[j >> 6] >> (j & 63)) & 1ull; }
// heads at the positions [0, j]
__device__ __forceinline__ int heads_upto(const uint64_t* sball, int j) {
  int h = 0;
  for (int k = 0; k < (j >> 6); ++k) h += __popcll(sball[k]);
  return h + __popcll(sball[j >> 6] & (~0ull >> (63 - (j & 63))));
}

template <int PASS>
__global__ __launch_bounds__(kThreads) void group_reduce_k(const double* __restrict__ x, int rows, int V,
                                                           const uint64_t* __restrict__ keys,
                                                           const long long* __restrict__ seg_off, long G, Out o,
                                                           uint64_t* __restrict__ part) {
  __shared__ double sv[kColBlock * kTile];
  __shared__ unsigned srow[kTile];
  __shared__ uint64_t sball[kChunks + 1];  // [kChunks]: bit 0 = the head flag behind a full tile
  __shared__ double slead[kColBlock][kWaves][kPartWords], stail[kColBlock][kWaves][kPartWords];
  __shared__ long long sg0;
  const long ntiles = ((long)rows + kTile - 1) / kTile;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  long nvalid = seg_off[G];
  if (!hx_guard(nvalid >= 0 && nvalid <= rows)) nvalid = 0;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long p0 = tile * kTile;
    const int nt = (int)(nvalid - p0 < kTile ? (nvalid - p0 > 0 ? nvalid - p0 : 0) : kTile);
    if (nt == 0) {  // behind the grouped rows (workgroup-uniform)
      if (threadIdx.x == 0) part_hdr(part, tile)[0] = part_hdr(part, tile)[1] = -1;
      continue;
    }
    for (int q = 0; q < kWaveChunks; ++q) {
      const int k = wv * kWaveChunks + q, j = k * 64 + lane;
      const long p = p0 + j;
      const bool in = j < nt;
      const uint64_t key = in ? keys[p] : 0ull;
      const uint64_t prev = (in && p > 0) ? keys[p - 1] : 0ull;
      unsigned row = (unsigned)key;
      if (!hx_guard(!in || row < (unsigned)rows)) row = 0;
      srow[j] = row;
      const uint64_t b = __ballot(in && (p == 0 || (key >> 32) != (prev >> 32)));
      if (lane == 0) sball[k] = b;
    }
    if (threadIdx.x == 0) {
      const long pe = p0 + nt;  // nt < kTile: the end of the grouped rows
      sball[kChunks] = (pe >= nvalid || (keys[pe] >> 32) != (keys[pe - 1] >> 32)) ? 1ull : 0ull;
      long lo = 0, hi = G;  // the group of p0: the last g with seg_off[g] <= p0
      while (hi - lo > 1) {
        const long mid = lo + ((hi - lo) >> 1);
        if (seg_off[mid] <= p0) lo = mid;
        else hi = mid;
      }
      sg0 = lo;
    }
    __syncthreads();
    const bool head0 = sball[0] & 1ull;
    const bool closed = nt < kTile ? true : (bool)(sball[kChunks] & 1ull);  // the tile's last run ends with the tile
    const long long gbase = sg0 - (head0 ? 1 : 0);                         // group of j = gbase + heads_upto(j)
    if (threadIdx.x == 0) {
      const bool any = heads_upto(sball, nt - 1) > 0;
      part_hdr(part, tile)[0] = head0 ? -1 : sg0;
      part_hdr(part, tile)[1] = (!closed && any) ? gbase + heads_upto(sball, nt - 1) : -1;
    }
    // this wave's span: ns positions, the first head at fh (kSpan: none), the run entering from the left is L long
    const int s0 = wv * kSpan;
    const int ns = nt - s0 < kSpan ? (nt - s0 > 0 ? nt - s0 : 0) : kSpan;
    int fh = kSpan;
    for (int q = kWaveChunks - 1; q >= 0; --q) {
      const uint64_t b = sball[wv * kWaveChunks + q];
      if (b) fh = q * 64 + __ffsll((long long)b) - 1;
    }
    const int L = fh < ns ? fh : ns;

    for (int c0 = 0; c0 < V; c0 += kColBlock) {
      const int cb = V - c0 < kColBlock ? V - c0 : kColBlock;
      __syncthreads();  // the earlier block's sv, slead and stail have been read
      for (int i = threadIdx.x; i < nt * cb; i += kThreads) {
        const int pos = i / cb;
        sv[(i - pos * cb) * kTile + pos] = x[(long)srow[pos] * V + c0 + (i - pos * cb)];
      }
      __syncthreads();
      for (int c = 0; c < cb; ++c) {
        Acc<PASS> carry = acc_none<PASS>();
        for (int q = 0; q < kWaveChunks; ++q) {
          const int k = wv * kWaveChunks + q, j = k * 64 + lane;
          const bool in = j < nt;
          const uint64_t ball = sball[k];
          const uint64_t below = ball & (~0ull >> (63 - lane));
          const int hpos = below ? 63 - __clzll((long long)below) : -1;  // this lane's run head in the 64, -1: earlier
          const long long g = gbase + heads_upto(sball, in ? j : 0);
          const double v = in ? sv[c * kTile + j] : nan;
          Acc<PASS> a = acc_none<PASS>();
          if (v == v) {
            if constexpr (PASS == 1) {
              a.v[0] = 1.0;
              a.v[1] = a.v[3] = a.v[4] = v;
            } else {
              const double d = hx_guard(g >= 0 && g < G) ? v - o.mean[g * V + c0 + c] : 0.0;
              a.v[0] = d;
              a.v[1] = d * d;
            }
          }
          const int start = hpos < 0 ? 0 : hpos;
#pragma unroll
          for (int s = 1; s < 64; s <<= 1) {
            Acc<PASS> u;
#pragma unroll
            for (int t = 0; t < Acc<PASS>::N; ++t) u.v[t] = __shfl_up(a.v[t], s, 64);
            if (lane - s >= start) a = comb<PASS>(u, a);
          }
          if (hpos < 0) a = comb<PASS>(carry, a);
#pragma unroll
          for (int t = 0; t < Acc<PASS>::N; ++t) carry.v[t] = __shfl(a.v[t], 63, 64);
          const int js = j - s0;  // position in the span
          if (in && js >= fh && (j == nt - 1 || head_at(sball, j + 1)))  // a run that starts in this span ends here
            emit<PASS>(a, true, j == nt - 1 ? closed : true, g, G, V, c0 + c, o, part, ntiles, tile);
          if (in && js == L - 1) {
#pragma unroll
            for (int t = 0; t < Acc<PASS>::N; ++t) slead[c][wv][t] = a.v[t];
          }
          if (in && js == ns - 1) {
#pragma unroll
            for (int t = 0; t < Acc<PASS>::N; ++t) stail[c][wv][t] = a.v[t];
          }
        }
      }
      __syncthreads();
      // the run that enters wave w's span from the left, if it ends there
      if (threadIdx.x < cb * kWaves) {
        const int c = threadIdx.x / kWaves, w = threadIdx.x % kWaves;
        const int ws0 = w * kSpan;
        const int wns = nt - ws0 < kSpan ? (nt - ws0 > 0 ? nt - ws0 : 0) : kSpan;
        int wfh = kSpan;
        for (int q = kWaveChunks - 1; q >= 0; --q) {
          const uint64_t b = sball[w * kWaveChunks + q];
          if (b) wfh = q * 64 + __ffsll((long long)b) - 1;
        }
        const int wL = wfh < wns ? wfh : wns;
        const int j = ws0 + wL - 1;
        if (wL > 0 && (j == nt - 1 || head_at(sball, j + 1))) {
          Acc<PASS> a = acc_none<PASS>();
          bool starts_here = false;
          for (int u = 0; u < w; ++u) {
            Acc<PASS> t;
#pragma unroll
            for (int q = 0; q < Acc<PASS>::N; ++q) t.v[q] = stail[c][u][q];
            bool has = false;
            for (int q = 0; q < kWaveChunks; ++q) has |= sball[u * kWaveChunks + q] != 0ull;
            a = has ? t : comb<PASS>(a, t);
            starts_here |= has;
          }
          Acc<PASS> l;
#pragma unroll
          for (int q = 0; q < Acc<PASS>::N; ++q) l.v[q] = slead[c][w][q];
          a = comb<PASS>(a, l);
          emit<PASS>(a, starts_here, j == nt - 1 ? closed : true, gbase + heads_upto(sball, j), G, V, c0 + c, o, part,
                     ntiles, tile);
        }
      }
    }
    __syncthreads();  // sball and srow are free for the next tile
  }
}

// a wave per tile whose partial 1 is set: that run's group, its partials in tile order
template <int PASS>
__global__ __launch_bounds__(kThreads) void group_finish_k(int rows, int V, const long long* __restrict__ seg_off,
                                                           long G, Out o, uint64_t* __restrict__ part) {
  const long ntiles = ((long)rows + kTile - 1) / kTile;
  const int lane = threadIdx.x & 63;
  for (long t = (long)blockIdx.x * kWaves + (threadIdx.x >> 6); t < ntiles; t += (long)gridDim.x * kWaves) {
    const long long g = part_hdr(part, t)[1];
    if (g < 0) continue;  // wave-uniform
    if (!hx_guard(g < G)) continue;
    const long tb = (seg_off[g + 1] - 1) / kTile;
    if (!hx_guard(tb > t && tb < ntiles)) continue;
    const long np = tb - t + 1;
    for (int c = 0; c < V; ++c) {
      Acc<PASS> a = acc_none<PASS>();
      for (long i = lane; i < np; i += 64) {
        hx_check(i == 0 || part_hdr(part, t + i)[0] == g);
        const double* p = part_val(part, ntiles, t + i, i == 0 ? 1 : 0, V, c);
        Acc<PASS> u;
#pragma unroll
        for (int q = 0; q < Acc<PASS>::N; ++q) u.v[q] = p[q];
        a = comb<PASS>(a, u);
      }
#pragma unroll
      for (int s = 1; s < 64; s <<= 1) {
        Acc<PASS> u;
#pragma unroll
        for (int q = 0; q < Acc<PASS>::N; ++q) u.v[q] = __shfl_xor(a.v[q], s, 64);
        a = (lane & s) ? comb<PASS>(u, a) : comb<PASS>(a, u);
      }
      if (lane == 0) write_group<PASS>(a, g, G, V, c, o);
    }
  }
}

}  // namespace groupagg

extern "C" int hopsx_group_tile() { return groupagg::kTile; }
extern "C" int hopsx_group_col_block() { return groupagg::kColBlock; }

extern "C" long hopsx_group_part_words(long rows, int V) {
  if (rows < 0 || rows > 0x7fffffffl || V < 0) return -1;
  return groupagg::tiles_of(rows) * 2 * (1 + groupagg::kPartWords * (long)V);
}

extern "C" int hopsx_group_keys64(const double* x, long rows, int cols, const int* key_cols, const long long* classes,
                                  int nkeys, const unsigned long long* comp, unsigned long long* keys,
                                  int max_workgroups, hipStream_t st) {
  using namespace groupagg;
  if (rows < 0 || rows > 0x7fffffffl || cols < 1 || nkeys < 1 || nkeys > kMaxKeys || max_workgroups < 0 || !key_cols ||
      !classes)
    return (int)hipErrorInvalidValue;
  KeyPlan plan = {};
  unsigned long long prod = 1;
  for (int k = nkeys - 1; k >= 0; --k) {
    if (key_cols[k] < 0 || key_cols[k] >= cols || classes[k] < 1 || classes[k] > 0x7fffffffll)
      return (int)hipErrorInvalidValue;
    plan.col[k] = key_cols[k];
    plan.radix[k] = (unsigned)classes[k];
    plan.mult[k] = (unsigned)prod;
    prod *= (unsigned long long)classes[k];
    if (prod >= (unsigned long long)kDropCode) return (int)hipErrorInvalidValue;  // the largest code stays below it
  }
  if (rows == 0) return (int)hipSuccess;
  if (!x || !comp || !keys) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(group_keys_k, dim3(grid_x((rows + kThreads - 1) / kThreads, max_workgroups)), dim3(kThreads), 0, st,
                     x, (int)rows, cols, nkeys, plan, (const uint64_t*)comp, (uint64_t*)keys);
  return (int)hipGetLastError();
}

// heads: ceil(rows / tile) uint32; seg_off int64 [rows + 1], first_row int64 [rows]: the first G + 1 resp. G are written
extern "C" int hopsx_group_heads64(const unsigned long long* keys, long rows, unsigned* heads, long long* seg_off,
                                   long long* first_row, long long* info, int max_workgroups, hipStream_t st) {
  using namespace groupagg;
  if (rows < 1 || rows > 0x7fffffffl || max_workgroups < 0 || !keys || !heads || !seg_off || !first_row || !info)
    return (int)hipErrorInvalidValue;
  const dim3 grid(grid_x(tiles_of(rows), max_workgroups)), block(kThreads);
  hipLaunchKernelGGL(group_heads_k<false>, grid, block, 0, st, (const uint64_t*)keys, (int)rows, heads, seg_off,
                     first_row, info);
  hipLaunchKernelGGL(group_headscan_k, dim3(1), block, 0, st, heads, (int)rows, info);
  hipLaunchKernelGGL(group_heads_k<true>, grid, block, 0, st, (const uint64_t*)keys, (int)rows, heads, seg_off,
                     first_row, info);
  return (int)hipGetLastError();
}

extern "C" int hopsx_group_reduce64(const double* x, long rows, int V, const unsigned long long* keys,
                                    const long long* seg_off, long G, unsigned long long* part, long long* count,
                                    double* sum, double* mn, double* mx, double* mean, double* var, int max_workgroups,
                                    hipStream_t st) {
  using namespace groupagg;
  if (rows < 0 || rows > 0x7fffffffl || V < 0 || G < 0 || G > rows || max_workgroups < 0)
    return (int)hipErrorInvalidValue;
  if (rows == 0 || V == 0 || G == 0) return (int)hipSuccess;
  if (!x || !keys || !seg_off || !part || !count || !sum || !mn || !mx || !mean) return (int)hipErrorInvalidValue;
  const Out o = {count, sum, mn, mx, mean, var};
  const long ntiles = tiles_of(rows);
  const dim3 grid(grid_x(ntiles, max_workgroups)), fgrid(grid_x((ntiles + kWaves - 1) / kWaves, max_workgroups));
  const dim3 block(kThreads);
  hipLaunchKernelGGL(group_reduce_k<1>, grid, block, 0, st, x, (int)rows, V, (const uint64_t*)keys, seg_off, G, o,
                     (uint64_t*)part);
  hipLaunchKernelGGL(group_finish_k<1>, fgrid, block, 0, st, (int)rows, V, seg_off, G, o, (uint64_t*)part);
  if (var) {
    hipLaunchKernelGGL(group_reduce_k<2>, grid, block, 0, st, x, (int)rows, V, (const uint64_t*)keys, seg_off, G, o,
                       (uint64_t*)part);
    hipLaunchKernelGGL(group_finish_k<2>, fgrid, block, 0, st, (int)rows, V, seg_off, G, o, (uint64_t*)part);
  }
  return (int)hipGetLastError();
}

HOPSX_DBG_TU(groupagg)
