// hopsx: per-column sort of fp64 feature columns and what the validation rules read off a sorted column (gfx950).
//
// x is fp64 [rows][cols], row-major, NaN = missing (the layout hopsx_column_stats64 takes); it is only read.
//
//   hopsx_column_sort64         keys[c][r] uint64, every column ascending, and count[c] = its non-NaN values.
//                               A key orders as the double does: -0.0 is folded onto +0.0, then with k the bits
//                               key = (k >> 63) ? ~k : (k | 1 << 63); every NaN becomes ~0, above +inf
//                               (0xFFF0000000000000), so the missing values are the tail of a sorted column.
//   hopsx_column_runs64         over the first count[c] keys: distinct (runs), unique (runs of length 1) and the
//                               entropy ln(n) - (sum over runs of L ln L) / n.
//   hopsx_column_order_values64 out[c][j] = the double behind keys[c][idx[c][j]].
//
// The sort is an LSD radix sort, 8-bit digits, all columns of a group in the same launches (column = grid.y):
//   encode_k    x -> keys (transpose), count[c] += valid (integer atomics)
//   ghist_k     the 8 digit histograms of every column (LDS counters, then integer atomics per workgroup)
//   plan_k      a digit whose histogram has one non-empty bin in EVERY column of the group is skipped (small integers
//               stored as doubles differ in their top two bytes only); writes per digit the side the keys are read from
//   per digit:  tilehist_k  digit histogram of every tile of kTile keys           -> th[c][digit][tile]
//               scan_k      th[c][digit][tile] := first output index of that tile's keys with that digit
//               scatter_k   ranks inside the tile that keep the input order (per 64 keys a match mask from 8 ballots,
//                           across the tile's 32 groups of 64 a prefix through LDS), the tile reordered in LDS, then
//                           written out so that neighbouring lanes write neighbouring keys of one digit
//   copy_k      when an odd number of digits ran the keys sit in the workspace: copy them to the output
// The kernels of a skipped digit are launched and return at once: the decision never reaches the host, so there is no
// synchronisation.  Every dependency is a kernel boundary; no workgroup waits for another.  Every pass is stable, and
// the sorted multiset is unique, so the output bits do not depend on the grid, the column grouping or the order in
// which atomics land.  Workgroups walk tiles grid-stride: max_workgroups only caps the grid.
//
// The two sides of the ping-pong are the caller's keys tensor and the workspace, so the workspace is one copy of a
// group's keys plus the histograms; columns are sorted in groups when that would exceed the cap.
//
// Run statistics: a run belongs to the tile that holds its head.  A thread owns 8 consecutive keys; a suffix minimum
// over the threads' first heads gives every head the next one, and the tile's last run finds its end by a binary
// search for the key's upper bound in the column.  Per-tile partials (integers, and L ln L summed in a fixed tree),
// then one workgroup per column adds the tiles in an order fixed by rows and kTile alone.  No float atomics.
#include "common.h"
#include "ops_api.h"

namespace colsort {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / HOPSX_WAVE;
constexpr int kPerThread = 8;
constexpr int kTile = kThreads * kPerThread;  // 2048 keys
constexpr int kGroups = kPerThread * kWaves;  // groups of 64 keys in a tile
constexpr int kDigits = 8;
constexpr int kBins = 256;
constexpr int kDefaultGrid = 4096;
constexpr int kPlanWords = 8;  // int32 plan[16] per column group: [p] = -1 skipped, 0 read keys, 1 read workspace;
                               // [8] = 1 when the sorted keys end in the workspace, [9] = mask of the digits run
constexpr uint64_t kNaNKey = ~0ull;

__device__ __forceinline__ uint64_t key_of(double v) {
  if (v != v) return kNaNKey;
  uint64_t k = (uint64_t)__double_as_longlong(v);
  if (k == 0x8000000000000000ull) k = 0ull;
  return (k >> 63) ? ~k : (k | 0x8000000000000000ull);
}
__device__ __forceinline__ double val_of(uint64_t key) {
  const uint64_t k = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
  return __longlong_as_double((long long)k);
}

// the layout of one group's workspace, in 64-bit words
struct Layout {
  long keys;   // rows * g
  long ghist;  // uint32 [g][8][256]
  long th;     // uint32 [g][256][ntiles]
  long plan;   // int32 [16]
  long total;
};
static inline long tiles_of(long rows) { return (rows + kTile - 1) / kTile; }
static inline Layout layout(long rows, long g) {
  Layout l;
  l.keys = 0;
  l.ghist = rows * g;
  l.th = l.ghist + g * (kDigits * kBins / 2);
  l.plan = l.th + g * ((kBins * tiles_of(rows) + 1) / 2);
  l.total = l.plan + kPlanWords;
  return l;
}
// columns per group under a cap of cap_bytes (0: 1 GiB); one column always goes
static inline int group_cols(long rows, int cols, long cap_bytes) {
  if (cap_bytes <= 0) cap_bytes = 1l << 30;
  const long per = layout(rows, 1).total - kPlanWords;
  long g = (cap_bytes / 8 - kPlanWords) / (per > 0 ? per : 1);
  if (g < 1) g = 1;
  if (g > cols) g = cols;
  return (int)g;
}

__global__ __launch_bounds__(kThreads) void encode_k(const double* __restrict__ x, int rows, int cols, int c0,
                                                     uint64_t* __restrict__ keys, unsigned long long* __restrict__ count) {
  const int c = c0 + blockIdx.y;
  const long ntiles = ((long)rows + kTile - 1) / kTile;
  uint64_t* out = keys + (long)c * rows;
  unsigned n = 0;  // wave-uniform
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const long r = tile * kTile + i * kThreads + threadIdx.x;
      bool valid = false;
      if (r < rows) {
        const uint64_t k = key_of(x[r * cols + c]);
        out[r] = k;
        valid = k != kNaNKey;
      }
      n += (unsigned)__popcll(__ballot(valid));
    }
  }
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(count + c, (unsigned long long)n);
}

__global__ __launch_bounds__(kThreads) void ghist_k(const uint64_t* __restrict__ keys, int rows, int c0,
                                                    unsigned* __restrict__ ghist) {
  __shared__ unsigned h[kDigits * kBins];
  const uint64_t* in = keys + (long)(c0 + blockIdx.y) * rows;
  const long ntiles = ((long)rows + kTile - 1) / kTile;
  for (int i = threadIdx.x; i < kDigits * kBins; i += kThreads) h[i] = 0u;
  __syncthreads();
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const long r = tile * kTile + i * kThreads + threadIdx.x;
      if (r < rows) {
        const uint64_t k = in[r];
#pragma unroll
        for (int p = 0; p < kDigits; ++p) atomicAdd(&h[p * kBins + (int)((k >> (8 * p)) & 255u)], 1u);
      }
    }
  }
  __syncthreads();
  unsigned* g = ghist + (long)blockIdx.y * (kDigits * kBins);
  for (int i = threadIdx.x; i < kDigits * kBins; i += kThreads)
    if (h[i]) atomicAdd(g + i, h[i]);
}

// one workgroup per column group
__global__ __launch_bounds__(kThreads) void plan_k(const unsigned* __restrict__ ghist, int rows, int g,
                                                   int* __restrict__ plan, int* __restrict__ mask_out) {
  __shared__ int full[kDigits];  // columns of the group whose digit p has one bin holding every row
  if (threadIdx.x < kDigits) full[threadIdx.x] = 0;
  __syncthreads();
  for (int c = 0; c < g; ++c)
    for (int p = 0; p < kDigits; ++p)
      if (ghist[((long)c * kDigits + p) * kBins + threadIdx.x] == (unsigned)rows) atomicAdd(&full[p], 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    int side = 0, mask = 0;
    for (int p = 0; p < kDigits; ++p) {
      const bool run = full[p] != g;
      plan[p] = run ? side : -1;
      if (run) {
        side ^= 1;
        mask |= 1 << p;
      }
    }
    plan[8] = side;
    plan[9] = mask;
    *mask_out = mask;
  }
}

__global__ __launch_bounds__(kThreads) void tilehist_k(const uint64_t* __restrict__ keys_out,
                                                       const uint64_t* __restrict__ keys_ws, int rows, int p,
                                                       const int* __restrict__ plan, unsigned* __restrict__ th) {
  const int side = plan[p];
  if (side < 0) return;
  __shared__ unsigned h[kBins];
  const uint64_t* in = (side ? keys_ws : keys_out) + (long)blockIdx.y * rows;
  const long ntiles = ((long)rows + kTile - 1) / kTile;
  unsigned* o = th + (long)blockIdx.y * kBins * ntiles;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    h[threadIdx.x] = 0u;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const long r = tile * kTile + i * kThreads + threadIdx.x;
      if (r < rows) atomicAdd(&h[(int)((in[r] >> (8 * p)) & 255u)], 1u);
    }
    __syncthreads();
    o[(long)threadIdx.x * ntiles + tile] = h[threadIdx.x];
    __syncthreads();
  }
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// a wave per digit: th[c][d][tile] := (keys of the column with a smaller digit) + (keys with digit d in earlier tiles)
__global__ __launch_bounds__(kThreads) void scan_k(const unsigned* __restrict__ ghist, int rows, int p,
                                                   const int* __restrict__ plan, unsigned* __restrict__ th) {
  if (plan[p] < 0) return;
  const int lane = threadIdx.x & 63, d = blockIdx.x * kWaves + (threadIdx.x >> 6);
  const long ntiles = ((long)rows + kTile - 1) / kTile;
  const unsigned* gh = ghist + ((long)blockIdx.y * kDigits + p) * kBins;
  unsigned base = 0;
  for (int j = lane; j < d; j += 64) base += gh[j];
  unsigned running = wave_sum_u32(base);
  unsigned* t = th + ((long)blockIdx.y * kBins + d) * ntiles;
  for (long t0 = 0; t0 < ntiles; t0 += 64) {
    const long i = t0 + lane;
    const unsigned v = i < ntiles ? t[i] : 0u;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned u = __shfl_up(inc, o, 64);
      if (lane >= o) inc += u;
    }
    if (i < ntiles) t[i] = running + inc - v;
    running += __shfl(inc, 63, 64);
  }
}

__global__ __launch_bounds__(kThreads) void scatter_k(uint64_t* __restrict__ keys_out, uint64_t* __restrict__ keys_ws,
                                                      int rows, int p, const int* __restrict__ plan,
                                                      const unsigned* __restrict__ th) {
  const int side = plan[p];
  if (side < 0) return;
  __shared__ uint64_t skey[kTile];
  __shared__ unsigned cnt[kGroups][kBins];  // keys with the digit in the earlier groups of 64 (after the prefix)
  __shared__ unsigned start[kBins];         // where the digit's keys begin in the reordered tile
  __shared__ unsigned gbase[kBins];         // where they begin in the output column
  const uint64_t* in = (side ? keys_ws : keys_out) + (long)blockIdx.y * rows;
  uint64_t* out = (side ? keys_out : keys_ws) + (long)blockIdx.y * rows;
  const long ntiles = ((long)rows + kTile - 1) / kTile;
  const unsigned* toff = th + (long)blockIdx.y * kBins * ntiles;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t below = (1ull << lane) - 1ull;

  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long r0 = tile * kTile;
    const int nt = (int)(rows - r0 < kTile ? rows - r0 : kTile);  // keys in this tile
#pragma unroll
    for (int g = 0; g < kGroups; ++g) cnt[g][tid] = 0u;
    gbase[tid] = toff[(long)tid * ntiles + tile];
    __syncthreads();

    uint64_t key[kPerThread];
    unsigned rank[kPerThread];
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const int j = i * kThreads + tid;
      const bool valid = j < nt;
      key[i] = valid ? in[r0 + j] : 0ull;
      const unsigned dg = (unsigned)(key[i] >> (8 * p)) & 255u;
      uint64_t m = __ballot(valid);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const bool bit = (dg >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        m &= bit ? bal : ~bal;
      }
      rank[i] = (unsigned)__popcll(m & below);
      if (valid && rank[i] == 0u) cnt[i * kWaves + wv][dg] = (unsigned)__popcll(m);
    }
    __syncthreads();
    {  // thread = digit: exclusive prefix over the groups, in tile order
      unsigned run = 0;
#pragma unroll
      for (int g = 0; g < kGroups; ++g) {
        const unsigned v = cnt[g][tid];
        cnt[g][tid] = run;
        run += v;
      }
      start[tid] = run;  // the digit's total for now
    }
    __syncthreads();
    {  // exclusive prefix over the 256 digit totals: wave scans, then the three wave sums
      const unsigned v = start[tid];
      unsigned inc = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
      }
      __shared__ unsigned wsum[kWaves];
      if (lane == 63) wsum[wv] = inc;
      __syncthreads();
      unsigned off = 0;
      for (int w = 0; w < wv; ++w) off += wsum[w];
      start[tid] = off + inc - v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const int j = i * kThreads + tid;
      if (j < nt) {
        const unsigned dg = (unsigned)(key[i] >> (8 * p)) & 255u;
        const unsigned pos = start[dg] + cnt[i * kWaves + wv][dg] + rank[i];
        if (hx_check(pos < (unsigned)nt)) skey[pos] = key[i];
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const int j = i * kThreads + tid;
      if (j < nt) {
        const uint64_t k = skey[j];
        const unsigned dg = (unsigned)(k >> (8 * p)) & 255u;
        const unsigned pos = gbase[dg] + ((unsigned)j - start[dg]);
        if (hx_guard(pos < (unsigned)rows)) out[pos] = k;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void copy_k(uint64_t* __restrict__ keys_out, const uint64_t* __restrict__ keys_ws,
                                                   long n, const int* __restrict__ plan) {
  if (plan[8] == 0) return;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads)
    keys_out[i] = keys_ws[i];
}

// ---- run statistics ----
// first index in [lo, n) of the sorted column whose key is above k
__device__ inline long upper_bound(const uint64_t* __restrict__ s, long lo, long n, uint64_t k) {
  long hi = n;
  while (lo < hi) {
    const long mid = lo + ((hi - lo) >> 1);
    if (s[mid] > k) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void runs_k(const uint64_t* __restrict__ keys, const long long* __restrict__ count,
                                                   int rows, uint64_t* __restrict__ part) {
  __shared__ int first[kThreads];
  __shared__ double sd[kThreads];
  __shared__ unsigned si[2][kThreads];
  const int c = blockIdx.y, tid = threadIdx.x;
  const uint64_t* s = keys + (long)c * rows;
  const long n = count[c];
  const long ntiles = ((long)rows + kTile - 1) / kTile;
  uint64_t* pd = part + ((long)c * 3 + 0) * ntiles;
  uint64_t* pu = part + ((long)c * 3 + 1) * ntiles;
  double* ps = (double*)(part + ((long)c * 3 + 2) * ntiles);
  constexpr int kNone = 0x7fffffff;

  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long t0 = tile * kTile;
    const long tend = t0 + kTile < n ? t0 + kTile : n;  // may lie below t0: nothing valid in the tile
    const long j0 = t0 + (long)tid * kPerThread;
    uint64_t k[kPerThread];
    uint64_t prev = (j0 > 0 && j0 < tend) ? s[j0 - 1] : 0ull;
    int head = 0, myfirst = kNone;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const long j = j0 + i;
      k[i] = j < tend ? s[j] : 0ull;
      const bool h = j < tend && (j == 0 || k[i] != prev);
      prev = k[i];
      if (h) {
        head |= 1 << i;
        if (myfirst == kNone) myfirst = tid * kPerThread + i;
      }
    }
    first[tid] = myfirst;
    __syncthreads();
    // first[t] := the first head at or after thread t's keys
#pragma unroll
    for (int o = 1; o < kThreads; o <<= 1) {
      const int a = first[tid], b = tid + o < kThreads ? first[tid + o] : kNone;
      __syncthreads();
      first[tid] = a < b ? a : b;
      __syncthreads();
    }
    int next = tid + 1 < kThreads ? first[tid + 1] : kNone;  // position in the tile of the next head, or none
    unsigned nd = 0, nu = 0;
    double sum = 0.0;
#pragma unroll
    for (int i = kPerThread - 1; i >= 0; --i) {
      if (!((head >> i) & 1)) continue;
      const long j = j0 + i;
      long end;
      if (next != kNone) end = t0 + next;
      else if (tend >= n) end = n;
      else end = upper_bound(s, tend, n, k[i]);  // the tile's last run goes on: at most one thread per tile
      const long len = end - j;
      nd += 1u;
      nu += len == 1 ? 1u : 0u;
      if (len > 1) sum += (double)len * log((double)len);
      next = tid * kPerThread + i;
    }
    sd[tid] = sum;
    si[0][tid] = nd;
    si[1][tid] = nu;
    __syncthreads();
#pragma unroll
    for (int o = kThreads / 2; o > 0; o >>= 1) {
      if (tid < o) {
        sd[tid] += sd[tid + o];
        si[0][tid] += si[0][tid + o];
        si[1][tid] += si[1][tid + o];
      }
      __syncthreads();
    }
    if (tid == 0) {
      pd[tile] = si[0][0];
      pu[tile] = si[1][0];
      ps[tile] = sd[0];
    }
    __syncthreads();
  }
}

// one workgroup per column: thread t adds tiles t, t + 256, ... in turn, then a fixed tree
__global__ __launch_bounds__(kThreads) void runs_sum_k(const uint64_t* __restrict__ part,
                                                       const long long* __restrict__ count, int rows,
                                                       long long* __restrict__ counts, double* __restrict__ entropy) {
  __shared__ double sd[kThreads];
  __shared__ unsigned long long si[2][kThreads];
  const int c = blockIdx.x, tid = threadIdx.x;
  const long ntiles = ((long)rows + kTile - 1) / kTile;
  const uint64_t* pd = part + ((long)c * 3 + 0) * ntiles;
  const uint64_t* pu = part + ((long)c * 3 + 1) * ntiles;
  const double* ps = (const double*)(part + ((long)c * 3 + 2) * ntiles);
  unsigned long long nd = 0, nu = 0;
  double sum = 0.0;
  for (long t = tid; t < ntiles; t += kThreads) {
    nd += pd[t];
    nu += pu[t];
    sum += ps[t];
  }
  sd[tid] = sum;
  si[0][tid] = nd;
  si[1][tid] = nu;
  __syncthreads();
#pragma unroll
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      sd[tid] += sd[tid + o];
      si[0][tid] += si[0][tid + o];
      si[1][tid] += si[1][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const long long n = count[c];
    counts[c * 3 + 0] = n;
    counts[c * 3 + 1] = (long long)si[0][0];
    counts[c * 3 + 2] = (long long)si[1][0];
    entropy[c] = n > 0 ? log((double)n) - sd[0] / (double)n : 0.0;
  }
}

__global__ __launch_bounds__(kThreads) void order_values_k(const uint64_t* __restrict__ keys, int rows, int cols, int m,
                                                           const long long* __restrict__ idx, double* __restrict__ out) {
  const long total = (long)cols * m;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long)gridDim.x * kThreads) {
    const long c = i / m;
    const long long j = idx[i];
    out[i] = hx_guard(j >= 0 && j < rows) ? val_of(keys[c * rows + j]) : __longlong_as_double(0x7ff8000000000000ll);
  }
}

static inline int grid_x(long ntiles, int g, int max_workgroups) {
  const long cap = max_workgroups > 0 ? max_workgroups : kDefaultGrid;
  long gx = cap / (g > 0 ? g : 1);
  if (gx < 1) gx = 1;
  if (gx > ntiles) gx = ntiles;
  return (int)gx;
}

}  // namespace colsort

extern "C" int hopsx_column_sort_tile() { return colsort::kTile; }

extern "C" int hopsx_column_sort_group_cols(long rows, int cols, long cap_bytes) {
  if (rows < 0 || rows > 0x7fffffffl || cols < 0) return -1;
  if (rows == 0 || cols == 0) return 0;
  return colsort::group_cols(rows, cols, cap_bytes);
}

extern "C" long hopsx_column_sort_ws_words(long rows, int cols, long cap_bytes) {
  if (rows < 0 || rows > 0x7fffffffl || cols < 0) return -1;
  if (rows == 0 || cols == 0) return 0;
  return colsort::layout(rows, colsort::group_cols(rows, cols, cap_bytes)).total;
}

extern "C" int hopsx_column_sort64(const double* x, long rows, int cols, unsigned long long* keys, long long* count,
                                   int* pass_mask, unsigned long long* ws, long ws_words, long cap_bytes,
                                   int max_workgroups, hipStream_t st) {
  using namespace colsort;
  if (rows < 0 || rows > 0x7fffffffl || cols < 0 || max_workgroups < 0) return (int)hipErrorInvalidValue;
  if (rows == 0 || cols == 0) return (int)hipSuccess;
  if (!x || !keys || !count || !pass_mask || !ws || ((uintptr_t)ws & 7)) return (int)hipErrorInvalidValue;
  const int G = group_cols(rows, cols, cap_bytes);
  if (ws_words < layout(rows, G).total) return (int)hipErrorInvalidValue;
  const long ntiles = tiles_of(rows);
  const int R = (int)rows;
  int e = hopsx_zero(count, (long)cols * 8, st);
  for (int c0 = 0, gi = 0; c0 < cols && !e; c0 += G, ++gi) {
    const int g = cols - c0 < G ? cols - c0 : G;
    const Layout l = layout(rows, g);
    uint64_t* kout = (uint64_t*)keys + (long)c0 * rows;
    uint64_t* kws = (uint64_t*)ws + l.keys;
    unsigned* ghist = (unsigned*)(ws + l.ghist);
    unsigned* th = (unsigned*)(ws + l.th);
    int* plan = (int*)(ws + l.plan);
    const dim3 grid(grid_x(ntiles, g, max_workgroups), g), block(kThreads);
    e = hopsx_zero(ghist, (long)g * kDigits * kBins * 4, st);
    if (e) break;
    hipLaunchKernelGGL(encode_k, grid, block, 0, st, x, R, cols, c0, (uint64_t*)keys, (unsigned long long*)count);
    hipLaunchKernelGGL(ghist_k, dim3(grid.x < 64u ? grid.x : 64u, g), block, 0, st, (const uint64_t*)keys, R, c0, ghist);
    hipLaunchKernelGGL(plan_k, dim3(1), block, 0, st, (const unsigned*)ghist, R, g, plan, pass_mask + gi);
    for (int p = 0; p < kDigits; ++p) {
      hipLaunchKernelGGL(tilehist_k, grid, block, 0, st, (const uint64_t*)kout, (const uint64_t*)kws, R, p,
                         (const int*)plan, th);
      hipLaunchKernelGGL(scan_k, dim3(kBins / kWaves, g), block, 0, st, (const unsigned*)ghist, R, p, (const int*)plan,
                         th);
      hipLaunchKernelGGL(scatter_k, grid, block, 0, st, kout, kws, R, p, (const int*)plan, (const unsigned*)th);
    }
    const long n = rows * g;
    long cg = (n + kThreads * 8 - 1) / (kThreads * 8);
    const long cap = max_workgroups > 0 ? max_workgroups : kDefaultGrid;
    if (cg > cap) cg = cap;
    hipLaunchKernelGGL(copy_k, dim3((unsigned)cg), block, 0, st, kout, (const uint64_t*)kws, n, (const int*)plan);
    e = (int)hipGetLastError();
  }
  return e;
}

// part: 3 * cols * ceil(rows / tile) 64-bit words
extern "C" int hopsx_column_runs64(const unsigned long long* keys, const long long* count, long rows, int cols,
                                   unsigned long long* part, long long* counts, double* entropy, int max_workgroups,
                                   hipStream_t st) {
  using namespace colsort;
  if (rows < 0 || rows > 0x7fffffffl || cols < 0 || max_workgroups < 0) return (int)hipErrorInvalidValue;
  if (cols == 0) return (int)hipSuccess;
  if (!count || !counts || !entropy || (rows > 0 && (!keys || !part))) return (int)hipErrorInvalidValue;
  const long ntiles = tiles_of(rows);
  if (rows > 0)
    hipLaunchKernelGGL(runs_k, dim3(grid_x(ntiles, cols, max_workgroups), cols), dim3(kThreads), 0, st,
                       (const uint64_t*)keys, count, (int)rows, (uint64_t*)part);
  hipLaunchKernelGGL(runs_sum_k, dim3(cols), dim3(kThreads), 0, st, (const uint64_t*)part, count, (int)rows, counts,
                     entropy);
  return (int)hipGetLastError();
}

extern "C" int hopsx_column_order_values64(const unsigned long long* keys, long rows, int cols, const long long* idx,
                                           int m, double* out, hipStream_t st) {
  using namespace colsort;
  if (rows < 0 || rows > 0x7fffffffl || cols < 0 || m < 0) return (int)hipErrorInvalidValue;
  if (rows == 0 || cols == 0 || m == 0) return (int)hipSuccess;
  if (!keys || !idx || !out) return (int)hipErrorInvalidValue;
  long g = ((long)cols * m + kThreads - 1) / kThreads;
  if (g > kDefaultGrid) g = kDefaultGrid;
  hipLaunchKernelGGL(order_values_k, dim3((unsigned)g), dim3(kThreads), 0, st, (const uint64_t*)keys, (int)rows, cols, m,
                     idx, out);
  return (int)hipGetLastError();
}

HOPSX_DBG_TU(colsort)
