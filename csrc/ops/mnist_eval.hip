// hopsx: forward-only inference of the flagship MNIST CNN over N resident uint8 images in ONE launch (gfx950).
//
// Model: mnist_persist.hip's (uint8 28x28 -> x * xscale + xshift -> Conv32 k2 relu -> Conv64 k2 relu ->
// MaxPool2 -> Dense128 relu -> Dense10 -> sparse softmax CE), dropout off: inference never drops.
//
// Partition: by IMAGE, not by pooled position.  A workgroup of 256 threads owns a tile of 32 images and
// walks the 169 pooled positions with the training kernel's per-position forward (4x4 input patch -> 3x3
// conv1 outputs (fp32 FMA, stored bf16) -> 128x64x128 conv2 MFMA + bias + relu -> bf16 -> 2x2 max-pool),
// and accumulates the [32 x 128] fc1 result in 16 fp32 MFMA accumulator registers per lane over the whole
// walk.  Nothing crosses workgroups, so there is no hand-off, no flag and no co-residency requirement: the
// grid is min(tiles, 2 x CUs) with a grid-stride loop over the tiles, and it runs on a partitioned GPU.
// Position p's fc1 weight slice (bf16 shadow, 128 rows of 128 B) is loaded into registers one position
// ahead (the loads stay in flight under the conv2 and fc1 MFMAs of the current position) and written to a
// single 18 KB LDS tile after the barrier that ends the previous fc1 product; the next 4x4 patch travels
// the same way.  The head (fc1 bias, relu, Dense10, softmax CE, argmax) runs once per tile from LDS.
//
// Numerics: the rounding points of the persistent kernel's forward (conv1 output, conv2 weight, conv2
// output and the fc1 weight in bf16; every accumulation in fp32; fc1 output, fc2, softmax and CE in fp32).
//
// Contract: an image's outputs depend only on that image and the weights — the MFMA rows of different
// images never mix, tail rows of the last tile are computed from zeros, never loaded past xs + N * 784 or
// ys + N, never stored and never counted.  `totals` = {sum of loss, hits} is deterministic: every tile
// writes a partial {fixed-tree sum of its 32 losses, hit count} and a second one-workgroup kernel sums the
// partials in an order that depends only on the number of tiles (no float atomics, no dependence on the
// grid size).  A label outside [0, 10) is reported through hx_guard, selects no logit, and gives loss 0 /
// hit 0.  The launch path allocates nothing, synchronises nothing and issues no memset: capture-safe.
#include "common.h"
#include "mnist_cnn.h"
#include "wg_prims.h"

namespace mnistev {
// Shared with the training kernel by construction, not by comment: the device vocabulary (f2bf_hw, lds8,
// mma32) and the model geometry (layer sizes, PH / NPOS / KIN, the W1S / W2S / C1S / PLS row strides of
// the images the MFMA fragments are read from).  The LDS map, the tile size and Args below are this
// kernel's own.
using namespace wgp;
using namespace mnist_cnn;

constexpr int TB = 32;  // images per tile
constexpr int IMG = 28 * 28;

// (mnist_cnn.h states the stride rule; this is what the addressing below relies on)
static_assert(KIN == NPOS * C2 && 2 * PH + 2 == 28, "13x13 pooled positions of 64 channels cover the image");
static_assert(W1S >= C2 && W2S >= 4 * C1 && C1S >= C1 && PLS >= C2, "a row holds its K extent");
static_assert(W1S % 8 == 0 && W2S % 8 == 0 && C1S % 8 == 0 && PLS % 8 == 0, "fragment reads are 16-B loads");

constexpr int HS = 132;  // f32 row stride of the fc1 output tile

// LDS map (bytes, every offset a multiple of 16)
constexpr int L_W1 = 0;                           // bf16 [128 n][W1S]   fc1 slice of the current position
constexpr int L_W2 = L_W1 + HID * W1S * 2;        // bf16 [64 co][W2S]   conv2 weights (OHWI rows)
constexpr int L_CW1 = L_W2 + C2 * W2S * 2;        // f32  [32][4]        conv1 weights
constexpr int L_CB1 = L_CW1 + C1 * 4 * 4;         // f32  [32]
constexpr int L_CB2 = L_CB1 + C1 * 4;             // f32  [64]
constexpr int L_FW2 = L_CB2 + C2 * 4;             // f32  [10][128]      fc2 weights
constexpr int L_FB1 = L_FW2 + NCLS * HID * 4;     // f32  [128]          fc1 bias
constexpr int L_FB2 = L_FB1 + HID * 4;            // f32  [16]           fc2 bias
constexpr int L_LOG = L_FB2 + 16 * 4;             // f32  [32 b][16]     logits of the tile
constexpr int L_XIN = L_LOG + TB * 16 * 4;        // f32  [32 b][16]     input patch
constexpr int L_POOL = L_XIN + TB * 16 * 4;       // bf16 [32 b][PLS]    pooled
constexpr int L_C1 = L_POOL + TB * PLS * 2;       // bf16 [32 b][9 pos][C1S] conv1 output
constexpr int LDS_BYTES = L_C1 + TB * 9 * C1S * 2;
constexpr int L_H = L_C1;                         // f32  [32 b][HS] fc1 output (aliases C1 after the walk)
static_assert(TB * HS * 4 <= TB * 9 * C1S * 2, "the fc1 output tile must fit the conv1 tile it aliases");
static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");
static_assert(NCLS * HID % 256 == 0 && C2 * 128 / 8 % 256 == 0, "parameter staging: whole passes of 256 threads");

struct Args {
  const float* master;       // arena fp32 parameters
  const bf16_raw* shadow;    // arena bf16 copy (conv2 / fc1 weights)
  long off[8];               // arena offsets: conv1.w conv1.b conv2.w conv2.b fc1.w fc1.b fc2.w fc2.b
  const unsigned char* xs;   // uint8 [n][28][28]
  const long long* ys;       // int64 [n] or null (logits only)
  long n;
  float* logits;             // [n][10]
  float* loss;               // [n]
  unsigned char* hit;        // [n]
  float* part;               // [ntiles][2] tile partials {loss sum, hits}
  float xscale, xshift;
  int ntiles;
};

__global__ __launch_bounds__(256, 2) void mnist_eval_k(const Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fq = lane >> 4;
  bf16_raw* W1 = (bf16_raw*)(smem + L_W1);
  bf16_raw* W2 = (bf16_raw*)(smem + L_W2);
  float* CW1 = (float*)(smem + L_CW1);
  float* CB1 = (float*)(smem + L_CB1);
  float* CB2 = (float*)(smem + L_CB2);
  float* FW2 = (float*)(smem + L_FW2);
  float* FB1 = (float*)(smem + L_FB1);
  float* FB2 = (float*)(smem + L_FB2);
  float* LOG = (float*)(smem + L_LOG);
  float* XIN = (float*)(smem + L_XIN);
  bf16_raw* POOL = (bf16_raw*)(smem + L_POOL);
  bf16_raw* A1 = (bf16_raw*)(smem + L_C1);
  float* H = (float*)(smem + L_H);

  // ---- parameters that stay in LDS for every tile of this workgroup (first read after a barrier below) ----
  {
    constexpr int NQ = C2 * 128 / 8 / 256;  // conv2 weights: 16-B pieces of the bf16 shadow
    bf16x8 wv[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) wv[q] = *(const bf16x8*)(a.shadow + a.off[2] + (tid + 256 * q) * 8);
    constexpr int NF = NCLS * HID / 256;
    float fv[NF];
#pragma unroll
    for (int q = 0; q < NF; ++q) fv[q] = a.master[a.off[6] + tid + 256 * q];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int j = (tid + 256 * q) * 8;
      *(bf16x8*)(W2 + (j >> 7) * W2S + (j & 127)) = wv[q];
    }
#pragma unroll
    for (int q = 0; q < NF; ++q) FW2[tid + 256 * q] = fv[q];
    if (tid < C1 * 4) CW1[tid] = a.master[a.off[0] + tid];
    if (tid < C1) CB1[tid] = a.master[a.off[1] + tid];
    if (tid < C2) CB2[tid] = a.master[a.off[3] + tid];
    if (tid < HID) FB1[tid] = a.master[a.off[5] + tid];
    if (tid < NCLS) FB2[tid] = a.master[a.off[7] + tid];
  }
  // input patch: thread -> (image xb, patch row xr, column pair xh); fc1 slice: thread -> (row, 64-B half)
  const int xb = tid >> 3, xr = (tid >> 1) & 3, xh = tid & 1;
  const bf16_raw* wrow = a.shadow + a.off[4] + (long)(tid >> 1) * KIN + (tid & 1) * 32;
  bf16_raw* wdst = W1 + (tid >> 1) * W1S + (tid & 1) * 32;

  for (long t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const long i0 = t * TB;
    const int nimg = a.n - i0 < TB ? (int)(a.n - i0) : TB;  // rows >= nimg: the tail, computed from zeros
    const bool xlive = xb < nimg;
    const unsigned char* xrow = a.xs + (i0 + (xlive ? xb : 0)) * IMG + xr * 28 + 2 * xh;
    auto xload = [&](int p) -> unsigned {
      const int ph = p / PH, pw = p - ph * PH;
      return xlive ? (unsigned)*(const unsigned short*)(xrow + 2 * ph * 28 + 2 * pw) : 0u;
    };
    unsigned xv = xload(0);
    bf16x8 wr[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) wr[q] = *(const bf16x8*)(wrow + 8 * q);
    f32x4 hacc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) hacc[i][jj] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int p = 0; p < NPOS; ++p) {
      XIN[xb * 16 + xr * 4 + 2 * xh] = (float)(xv & 0xFFu) * a.xscale + a.xshift;
      XIN[xb * 16 + xr * 4 + 2 * xh + 1] = (float)(xv >> 8) * a.xscale + a.xshift;
      __syncthreads();  // every wave is past the previous position's fc1 product: W1 is free
#pragma unroll
      for (int q = 0; q < 4; ++q) *(bf16x8*)(wdst + 8 * q) = wr[q];
      if (p + 1 < NPOS) {  // the next position's patch and fc1 slice: in flight until the next iteration
        xv = xload(p + 1);
#pragma unroll
        for (int q = 0; q < 4; ++q) wr[q] = *(const bf16x8*)(wrow + (p + 1) * C2 + 8 * q);
      }
      // ---- conv1 (VALU): 32 images x 3x3 positions x 32 channels ----
      {
        const int ci = tid & 31, bg = tid >> 5;
        const float k0 = CW1[ci * 4 + 0], k1 = CW1[ci * 4 + 1], k2 = CW1[ci * 4 + 2], k3 = CW1[ci * 4 + 3];
        const float bias = CB1[ci];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int b = bg * 4 + u;
          const float* xi = XIN + b * 16;
#pragma unroll
          for (int py = 0; py < 3; ++py)
#pragma unroll
            for (int px = 0; px < 3; ++px) {
              float v = bias;
              v = fmaf(xi[py * 4 + px], k0, v);
              v = fmaf(xi[py * 4 + px + 1], k1, v);
              v = fmaf(xi[(py + 1) * 4 + px], k2, v);
              v = fmaf(xi[(py + 1) * 4 + px + 1], k3, v);
              A1[(b * 9 + py * 3 + px) * C1S + ci] = f2bf_hw(fmaxf(v, 0.f));
            }
        }
      }
      __syncthreads();
      // ---- conv2 (MFMA, rows (b, q) = b*4 + q, k = tap*32 + ci) + bias + relu -> bf16 -> max-pool ----
      {
        f32x4 acc[2][4];
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[ii][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int di = kk >> 1, dj = kk & 1;
          bf16x8 af[2];
#pragma unroll
          for (int ii = 0; ii < 2; ++ii) {
            const int b = 4 * (2 * w + ii) + (fr >> 2), q = fr & 3;
            const int pos = ((q >> 1) + di) * 3 + (q & 1) + dj;
            af[ii] = lds8(A1 + (b * 9 + pos) * C1S + fq * 8);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bf16x8 bfr = lds8(W2 + (j * 16 + fr) * W2S + kk * 32 + fq * 8);
#pragma unroll
            for (int ii = 0; ii < 2; ++ii) acc[ii][j] = mma32(af[ii], bfr, acc[ii][j]);
          }
        }
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int b = 4 * (2 * w + ii) + fq, co = j * 16 + fr;
            const float bias = CB2[co];
            float best = 0.f;  // the window's values are relu outputs
#pragma unroll
            for (int r = 0; r < 4; ++r) best = fmaxf(best, bf2f(f2bf_hw(fmaxf(acc[ii][j][r] + bias, 0.f))));
            POOL[b * PLS + co] = f2bf_hw(best);
          }
      }
      __syncthreads();
      // ---- fc1: this position's 64 inputs, accumulated over the walk (rows = images, cols = hidden) ----
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8 af[2], bfr[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) af[i] = lds8(POOL + (i * 16 + fr) * PLS + kk * 32 + fq * 8);
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) bfr[jj] = lds8(W1 + ((2 * w + jj) * 16 + fr) * W1S + kk * 32 + fq * 8);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) hacc[i][jj] = mma32(af[i], bfr[jj], hacc[i][jj]);
      }
    }
    // ---- head: fc1 bias + relu (fp32) -> LDS (the conv1 tile's last readers passed the barrier above) ----
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int b = i * 16 + fq * 4 + r, n = (2 * w + jj) * 16 + fr;
          H[b * HS + n] = fmaxf(hacc[i][jj][r] + FB1[n], 0.f);
        }
    __syncthreads();
    // Dense10: thread -> (image, class) pairs e and e + 256 of the tile's 320, a serial fp32 dot product
    for (int e = tid; e < TB * NCLS; e += 256) {
      const int b = e / NCLS, c = e - b * NCLS;
      float v = 0.f;
#pragma unroll 8
      for (int k = 0; k < HID; ++k) v = fmaf(H[b * HS + k], FW2[c * HID + k], v);
      v += FB2[c];
      LOG[b * 16 + c] = v;
      if (b < nimg) a.logits[i0 * NCLS + e] = v;
    }
    __syncthreads();
    if (a.ys && tid < 64) {  // softmax CE + argmax: lane b < 32 owns image b
      const int b = lane & (TB - 1);
      const bool live = lane < nimg;  // (nimg <= 32)
      const long long y = live ? a.ys[i0 + lane] : 0;
      bool ok = false;
      if (live) ok = hx_guard((unsigned long long)y < (unsigned long long)NCLS);  // the label selects on-chip only
      float z[NCLS];
#pragma unroll
      for (int c = 0; c < NCLS; ++c) z[c] = LOG[b * 16 + c];
      float m = z[0];
#pragma unroll
      for (int c = 1; c < NCLS; ++c) m = fmaxf(m, z[c]);
      float se = 0.f, zy = 0.f;
      int am = NCLS;
#pragma unroll
      for (int c = NCLS - 1; c >= 0; --c) {
        if (z[c] == m) am = c;  // the first maximum
        if ((long long)c == y) zy = z[c];
      }
#pragma unroll
      for (int c = 0; c < NCLS; ++c) se += __expf(z[c] - m);
      float l = ok ? __logf(se) + m - zy : 0.f;
      int h = ok && (long long)am == y ? 1 : 0;
      if (live) {
        a.loss[i0 + lane] = l;
        a.hit[i0 + lane] = (unsigned char)h;
      } else {
        l = 0.f;
        h = 0;
      }
      // the tile's partial: a fixed tree over the 32 images (the tail adds exact zeros)
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) {
        l += __shfl_xor(l, o, 64);
        h += __shfl_xor(h, o, 64);
      }
      if (lane == 0) {
        a.part[2 * t] = l;
        a.part[2 * t + 1] = (float)h;
      }
    }
    // (no barrier: the next tile's first writes to H's memory and to LOG come after its own barriers)
  }
}

// totals = {sum of the tiles' loss partials, hits}: thread k sums tiles k, k + 256, ... in that order, then a
// fixed LDS tree — an order that depends only on the number of tiles; the hits are summed as integers
__global__ __launch_bounds__(256) void mnist_eval_totals_k(const float* part, int ntiles, float* totals) {
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

}  // namespace mnistev

HOPSX_DBG_TU(mnist_eval)

// ptrs: master shadow xs ys(0 = logits only) logits loss hit totals part([ceil(n / 32)][2] floats)
// iv:   off[8] n max_workgroups(0 = 2 per CU)
// fv:   xscale xshift
extern "C" int hopsx_mnist_eval(const uint64_t* p, int np, const long* iv, int ni, const float* fv, int nf,
                                hipStream_t st) {
  using namespace mnistev;
  if (np < 9 || ni < 10 || nf < 2) return (int)hipErrorInvalidValue;
  const long n = iv[8];
  if (n < 0) return (int)hipErrorInvalidValue;
  if (n == 0) return (int)hipSuccess;
  const long ntiles = (n + TB - 1) / TB;
  if (ntiles > 0x7fffffffL) return (int)hipErrorInvalidValue;
  Args a{};
  a.master = (const float*)p[0];
  a.shadow = (const bf16_raw*)p[1];
  a.xs = (const unsigned char*)p[2];
  a.ys = (const long long*)p[3];
  a.logits = (float*)p[4];
  a.loss = (float*)p[5];
  a.hit = (unsigned char*)p[6];
  float* totals = (float*)p[7];
  a.part = (float*)p[8];
  for (int k = 0; k < 8; ++k) a.off[k] = iv[k];
  a.n = n;
  a.ntiles = (int)ntiles;
  a.xscale = fv[0];
  a.xshift = fv[1];
  if (!a.master || !a.shadow || !a.xs || !a.logits) return (int)hipErrorInvalidValue;
  if (a.ys && (!a.loss || !a.hit || !totals || !a.part)) return (int)hipErrorInvalidValue;
  // 16-B loads of the bf16 shadow (arena offsets are 64-element aligned), 2-B loads of the images
  if ((p[1] & 15) || (a.off[2] & 7) || (a.off[4] & 7) || (p[2] & 1)) return (int)hipErrorInvalidValue;
  for (int k = 0; k < 8; ++k)
    if (a.off[k] < 0) return (int)hipErrorInvalidValue;
  int dev = 0, cus = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess || cus < 1) return (int)(e != hipSuccess ? e : hipErrorInvalidDevice);
  long grid = iv[9] > 0 ? iv[9] : 2L * cus;
  if (grid > ntiles) grid = ntiles;
  static bool attr[64] = {};  // per device: the kernel's dynamic LDS exceeds the 64 KB default limit
  if (dev < 0 || dev >= 64 || !attr[dev]) {
    e = hipFuncSetAttribute((const void*)mnist_eval_k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    if (e != hipSuccess) return (int)e;
    if (dev >= 0 && dev < 64) attr[dev] = true;
  }
  hipLaunchKernelGGL(mnist_eval_k, dim3((unsigned)grid), dim3(256), LDS_BYTES, st, a);
  if (a.ys) hipLaunchKernelGGL(mnist_eval_totals_k, dim3(1), dim3(256), 0, st, a.part, a.ntiles, totals);
  return (int)hipGetLastError();
}

extern "C" int hopsx_mnist_eval_tile() { return mnistev::TB; }
