// hopsx: the deterministic totals kernel of the one-launch evaluators (mnist_eval.hip, cnn_eval.hip).
#pragma once
#include "common.h"

namespace evtot {

// totals = {sum of the tiles' loss partials, hits}: thread k sums tiles k, k + 256, ... in that order, then a
// fixed LDS tree — an order that depends only on the number of tiles; the hits are summed as integers
static __global__ __launch_bounds__(256) void eval_totals_k(const float* part, int ntiles, float* totals) {
  __shared__ float sl[256];
  __shared__ int sh[256];
  const int tid = threadIdx.x;
  float l = 0.f;
  int h = 0;
  for (int k = tid; k < ntiles; k += 256) {
    l += part[2 * k];
    h += (int)part[2 * k + 1];
  }
  sl[tid] = l;
  sh[tid] = h;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      sl[tid] += sl[tid + s];
      sh[tid] += sh[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    totals[0] = sl[0];
    totals[1] = (float)sh[0];
  }
}

}  // namespace evtot
