// hopsx: row softmax + top-k of classifier logits (gfx950), the tail of the inference path.
//
// For every row of contiguous logits [B][C] (fp32 or bf16): ids[B][k] = the classes of the k largest logits,
// largest first, the lower class first among equal values; scores[B][k] = their softmax probabilities
// exp(z - m) / sum_c exp(z_c - m), m the row maximum.  1 <= k <= 8, k <= C.
//
// Selection is integer work only.  A logit's fp32 bits map to a uint32 that orders as the floats do (-0.0 folded onto
// +0.0, bf16 widened exactly); with 0x7fffffff - class in the low word the 64-bit composites of a row are distinct, their
// maximum is the largest value at its lowest class, and the (j+1)-th pick is the largest composite below the j-th.  No
// rounding takes part, so the ids are exact; a row with NaN or +inf still yields k distinct classes inside [0, C)
// (its scores are unspecified).  A -inf class scores exp(-inf) = 0.
//
// Routes, chosen from C alone (hopsx_softmax_topk_path):
//   0  wave per row, C <= 1024: a lane's share is at most 16 values (fp32: 4 loads of 16 bytes, bf16: 2), kept in
//      registers as keys; each pick is one scan of those registers and a 64-lane max.  4 rows per workgroup,
//      no LDS, no barrier.
//   1  workgroup (256 threads) per row, C > 1024: every thread walks its 16-byte chunks once, keeping its own 8 best
//      composites in a sorted register list; a pick is a wave max + 4 LDS words, and the thread whose head won pops
//      it.  A second walk of the row (from cache) takes the sum.
// The element -> lane / register mapping is fixed by C: chunk c of 16 bytes belongs to thread c % threads.  A chunk
// is one 16-byte load when the row's base is 16-byte aligned and the chunk lies inside the row, and element loads
// otherwise (a row of an odd-C tensor, the row's tail), so alignment changes the loads and never the order of the
// sum: per-thread partials in chunk order, wave_sum, then (route 1) the four wave sums as (s0 + s1) + (s2 + s3).  A
// row's outputs are therefore the same bits for any B, any position in the batch and any grid.
//
// The exponential is this file's own exp_neg (x * log2e as a rounded product plus its low part, v_exp_f32 on the
// fraction, ldexp: about 1 ulp), not expf and not __expf: the scores are held to 8 x the error of an fp32 softmax.
// __expf's argument rounding alone is |z - m| * 2^-24 relative; and under the library's -ffp-contract=fast hipcc
// compiles expf's own expansion no better — it fuses "product - rint(product)" into fma(x, log2e, -rint), which
// already holds the low part, then adds the low part again: 2.5e-6 relative at x = -51.5 measured on an MI355X,
// 20 x the fp32 softmax's error.  exp_neg pins the rounded product so that nothing is fused into it.  At 1000
// classes per row the exponentials are not what the kernel's time goes to.
//
// The launcher allocates nothing, synchronises nothing and issues no memset: one kernel node under capture.
#include "common.h"
#include "ops_api.h"

namespace topk {

constexpr int kMaxK = 8;
constexpr int kWaveMaxC = 1024;   // route 0 up to here: 16 keys per lane
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / HOPSX_WAVE;
constexpr int kDefaultGrid = 2048;  // 256 CUs x 8 resident workgroups of 256 threads

template <typename T> struct Chunk;
template <> struct Chunk<float> { static constexpr int N = 4; };
template <> struct Chunk<bf16_raw> { static constexpr int N = 8; };

// fp32 bits -> uint32 ordered as the floats are; and back
__device__ __forceinline__ uint32_t key_of(uint32_t u) {
  if (u == 0x80000000u) u = 0u;  // -0.0 == +0.0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float val_of(uint32_t key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}
// never 0 (idx <= 2^31 - 2) and never all ones: 0 stands for "nothing", ~0 for "no pick yet"
__device__ __forceinline__ uint64_t comp_of(uint32_t key, int idx) {
  return ((uint64_t)key << 32) | (uint64_t)(0x7fffffffu - (uint32_t)idx);
}
__device__ __forceinline__ int idx_of(uint64_t comp) { return (int)(0x7fffffffu - (uint32_t)comp); }
__device__ __forceinline__ uint32_t key_part(uint64_t comp) { return (uint32_t)(comp >> 32); }

// exp(x) for x <= 0, -inf and NaN included (see the header)
__device__ __forceinline__ float exp_neg(float x) {
  const float c = 0x1.715476p+0f, cc = 0x1.4ae0bep-26f;  // log2(e) = c + cc to 49 bits
  if (x < -104.f) return 0.f;  // below half the least subnormal (and -inf, whose low part would be inf - inf)
  float ph = x * c;
  asm volatile("" : "+v"(ph));  // the ROUNDED product from here on: no fma(x, c, ...) in its place
  const float pl = fmaf(x, cc, fmaf(x, c, -ph));
  const float e = rintf(ph);
  return ldexpf(__builtin_amdgcn_exp2f((ph - e) + pl), (int)e);
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t t = __shfl_xor((unsigned long long)v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

// keys of the row's elements [e0, e0 + N); elements at or past C get key 0 (callers test the index themselves)
__device__ __forceinline__ void load_keys(const float* row, long e0, int C, bool vec, uint32_t* key) {
  if (vec && e0 + 4 <= C) {
    const f32x4 v = *(const f32x4*)(row + e0);
#pragma unroll
    for (int j = 0; j < 4; ++j) key[j] = key_of(__float_as_uint(v[j]));
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) key[j] = e0 + j < C ? key_of(__float_as_uint(row[e0 + j])) : 0u;
  }
}
__device__ __forceinline__ void load_keys(const bf16_raw* row, long e0, int C, bool vec, uint32_t* key) {
  if (vec && e0 + 8 <= C) {
    const bf16x8 v = *(const bf16x8*)(row + e0);
#pragma unroll
    for (int j = 0; j < 8; ++j) key[j] = key_of((uint32_t)(uint16_t)v[j] << 16);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) key[j] = e0 + j < C ? key_of((uint32_t)row[e0 + j] << 16) : 0u;
  }
}

// ---- route 0: a wave per row, NP passes of 64 chunks ----
template <typename T, int NP>
__global__ __launch_bounds__(kThreads) void softmax_topk_wave_k(const T* __restrict__ x, int* __restrict__ ids,
                                                                 float* __restrict__ scores, int B, int C, int k) {
  constexpr int N = Chunk<T>::N, E = NP * N;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (long row = (long)blockIdx.x * kWaves + wv; row < B; row += (long)gridDim.x * kWaves) {
    const T* r = x + row * C;
    const bool vec = ((uintptr_t)r & 15) == 0;
    uint32_t key[E];
#pragma unroll
    for (int p = 0; p < NP; ++p) load_keys(r, (long)(p * 64 + lane) * N, C, vec, key + p * N);

    uint64_t prev = ~0ull;
    int my_id = 0;
    uint32_t my_key = 0, top_key = 0;
    for (int j = 0; j < k; ++j) {
      uint64_t best = 0;
#pragma unroll
      for (int s = 0; s < E; ++s) {
        const int idx = ((s / N) * 64 + lane) * N + (s % N);
        const uint64_t c = idx < C ? comp_of(key[s], idx) : 0ull;
        best = (c < prev && c > best) ? c : best;
      }
      best = wave_max_u64(best);  // never 0: k <= C leaves an element below prev
      if (j == 0) top_key = key_part(best);
      if (lane == j) {
        my_id = idx_of(best);
        my_key = key_part(best);
      }
      prev = best;
    }
    const float m = val_of(top_key);
    float part = 0.f;
#pragma unroll
    for (int s = 0; s < E; ++s) {
      const int idx = ((s / N) * 64 + lane) * N + (s % N);
      if (idx < C) part += exp_neg(val_of(key[s]) - m);
    }
    const float sum = wave_sum(part);
    if (lane < k) {
      ids[row * k + lane] = my_id;
      scores[row * k + lane] = exp_neg(val_of(my_key) - m) / sum;
    }
  }
}

// ---- route 1: a workgroup per row ----
template <typename T>
__global__ __launch_bounds__(kThreads) void softmax_topk_wg_k(const T* __restrict__ x, int* __restrict__ ids,
                                                               float* __restrict__ scores, int B, int C, int k) {
  constexpr int N = Chunk<T>::N;
  __shared__ uint64_t s_best[kMaxK][kWaves];  // one line per pick: no reuse inside a row
  __shared__ float s_sum[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long nchunk = ((long)C + N - 1) / N;
  for (long row = blockIdx.x; row < B; row += gridDim.x) {
    const T* r = x + row * C;
    const bool vec = ((uintptr_t)r & 15) == 0;
    uint64_t list[kMaxK];  // this thread's best composites, descending; 0 = empty
#pragma unroll
    for (int i = 0; i < kMaxK; ++i) list[i] = 0;
    for (long c = tid; c < nchunk; c += kThreads) {
      uint32_t key[N];
      load_keys(r, c * N, C, vec, key);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const long idx = c * N + j;
        uint64_t v = idx < C ? comp_of(key[j], (int)idx) : 0ull;
        if (v > list[kMaxK - 1]) {
#pragma unroll
          for (int i = 0; i < kMaxK; ++i) {
            const bool gt = v > list[i];
            const uint64_t t = gt ? list[i] : v;
            list[i] = gt ? v : list[i];
            v = t;
          }
        }
      }
    }
    int my_id = 0;
    uint32_t my_key = 0, top_key = 0;
    for (int j = 0; j < k; ++j) {
      const uint64_t w = wave_max_u64(list[0]);
      if (lane == 0) s_best[j][wv] = w;
      __syncthreads();
      uint64_t best = s_best[j][0];
#pragma unroll
      for (int i = 1; i < kWaves; ++i) best = s_best[j][i] > best ? s_best[j][i] : best;
      if (list[0] == best) {  // one thread: composites are distinct, and best != 0 since k <= C
#pragma unroll
        for (int i = 0; i + 1 < kMaxK; ++i) list[i] = list[i + 1];
        list[kMaxK - 1] = 0;
      }
      if (j == 0) top_key = key_part(best);
      if (tid == j) {
        my_id = idx_of(best);
        my_key = key_part(best);
      }
    }
    const float m = val_of(top_key);
    float part = 0.f;
    for (long c = tid; c < nchunk; c += kThreads) {
      uint32_t key[N];
      load_keys(r, c * N, C, vec, key);
#pragma unroll
      for (int j = 0; j < N; ++j)
        if (c * N + j < C) part += exp_neg(val_of(key[j]) - m);
    }
    part = wave_sum(part);
    if (lane == 0) s_sum[wv] = part;
    __syncthreads();
    const float sum = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    if (tid < k) {
      ids[row * k + tid] = my_id;
      scores[row * k + tid] = exp_neg(val_of(my_key) - m) / sum;
    }
    __syncthreads();  // the next row writes s_best / s_sum
  }
}

template <typename T>
static void launch(int path, const void* x, int* ids, float* scores, int B, int C, int k, int cap, hipStream_t st) {
  constexpr int N = Chunk<T>::N;
  const T* xp = (const T*)x;
  if (path == 1) {
    const int grid = B < cap ? B : cap;
    hipLaunchKernelGGL(softmax_topk_wg_k<T>, dim3(grid), dim3(kThreads), 0, st, xp, ids, scores, B, C, k);
    return;
  }
  const int groups = (B + kWaves - 1) / kWaves;
  const dim3 grid(groups < cap ? groups : cap), block(kThreads);
  // passes of 64 chunks: 1, 2, or (fp32 only) 4 — every C of route 0 must fit the widest instantiation
  constexpr int kMaxNP = N == 4 ? 4 : 2;
  static_assert(kWaveMaxC <= 64 * N * kMaxNP, "route 0 has no kernel for a row this long");
  const int np = (C + 64 * N - 1) / (64 * N);
  if (np <= 1) {
    hipLaunchKernelGGL((softmax_topk_wave_k<T, 1>), grid, block, 0, st, xp, ids, scores, B, C, k);
  } else if (np == 2) {
    hipLaunchKernelGGL((softmax_topk_wave_k<T, 2>), grid, block, 0, st, xp, ids, scores, B, C, k);
  } else {
    hipLaunchKernelGGL((softmax_topk_wave_k<T, kMaxNP>), grid, block, 0, st, xp, ids, scores, B, C, k);
  }
}

}  // namespace topk

// The launcher's route, stated once: 0 wave per row, 1 workgroup per row, -2 refused (nothing would be launched)
extern "C" int hopsx_softmax_topk_path(const void* x, int is_bf16, int B, int C, int k, const int* ids,
                                       const float* scores) {
  if (!x || !ids || !scores || (is_bf16 != 0 && is_bf16 != 1)) return -2;
  if (B < 0 || C < 1 || k < 1 || k > topk::kMaxK || k > C) return -2;
  if (((uintptr_t)x & (is_bf16 ? 1 : 3)) || ((uintptr_t)ids & 3) || ((uintptr_t)scores & 3)) return -2;
  return C <= topk::kWaveMaxC ? 0 : 1;
}

extern "C" int hopsx_softmax_topk(const void* x, int is_bf16, int B, int C, int k, int* ids, float* scores,
                                  int max_workgroups, hipStream_t st) {
  const int path = hopsx_softmax_topk_path(x, is_bf16, B, C, k, ids, scores);
  if (path < 0 || max_workgroups < 0) return (int)hipErrorInvalidValue;
  if (B == 0) return (int)hipSuccess;
  const int cap = max_workgroups > 0 ? max_workgroups : topk::kDefaultGrid;
  if (is_bf16)
    topk::launch<bf16_raw>(path, x, ids, scores, B, C, k, cap, st);
  else
    topk::launch<float>(path, x, ids, scores, B, C, k, cap, st);
  return (int)hipGetLastError();
}

HOPSX_DBG_TU(topk)
