// The whole training step of a small Dense stack (the Titanic DNN of BASELINE config 4, the simulated-data
// MLP, the maggy regressor) in ONE workgroup: forward, loss, backward, Adam / AdamW, step counter and batch
// cursor, `nsteps` steps a launch over an HBM-resident epoch.
//
// Such a step is < 40 k MACs an example: layer by layer it is ~17 launches of hand-off latency and no
// arithmetic.  Like taxi_step.hip this kernel keeps ONE workgroup (512 threads) on one dependent chain with
// the model on chip, but its geometry is a RUNTIME layer table (1..8 Linear layers with bias, every width
// 1..64, last width 1, batch 1..64), so one binary serves every Dense-only stack of the zoo:
//
//   * mixed precision like the rest of the framework: activations, gradients and weights are bf16 images in
//     LDS (one image per tensor, row stride an odd multiple of 16 elements, widths zero-padded to 16), fp32
//     accumulation in `v_mfma_f32_16x16x32_bf16` (K chunks of 32) and `16x16x16` (the K tail and dW), fp32
//     master weights and Adam moments.  Row reads feed the forward and dX products, `ds_read_b64_tr_b16`
//     transposed reads dX's W operand and both dW operands.
//   * "tile waves" 0..ceil(B/16)-1 each own one 16-row batch tile: its forward through every hidden layer,
//     the last layer (width 1: a dot product with the bf16-rounded weights, no MFMA), the loss and the logit
//     gradient run with no workgroup barrier; then one dX layer per backward phase.  All 8 waves share the dW
//     tiles of the layer whose G was finished one phase earlier, the waves without a batch tile first.
//     db is a dW tile too: the MFMA of a constant ones operand with G (no ones column in the images);
//     biases are applied in fp32 in the forward epilogue.  L barriers a step for L layers.
//   * optimizer state: form (b) of the two the design allowed.  The lane whose accumulator receives a
//     parameter's gradient owns that parameter for the whole launch (tile -> wave map from the layer table),
//     and its fp32 w, m, v sit in an LDS copy of the arena span next to the images, loaded and stored
//     coalesced once a launch.  Form (a), registers, needs 3 x 4 x rounds statically indexed registers a
//     lane, with the round count a compile-time maximum: 168 for seven 64 x 64 layers, which does not leave
//     0 scratch at 256 registers a lane.  Where the span does not fit LDS beside the images (the Titanic DNN
//     at batch 64; seven 64 x 64 layers, whose images alone take 156 KB) the owner lane updates w, m, v in
//     place in the arena instead: still one lane per element and no hand-off, the traffic stays in this CU's
//     caches.  `hopsx_mlp_step_ok` computes the budget and says which; what fits neither way is refused.
//   * a layer's new bf16 image is written one phase after its dW, once its dX has read the old one.
//   * every sum has a fixed order (MFMA accumulation over batch tiles in order, shuffles, ordered loops): no
//     float atomics, so an nsteps launch equals nsteps one-step launches bit for bit.
//   * the batch: fp32 xs[nbatch][B][F] / ys[nbatch][B] read with plain loads (no alignment assumed),
//     converted to bf16 into a double-buffered zero-padded input image; the next batch's loads are in flight
//     during the step.  Rows >= B are zero in every activation and gradient image.
//   * `trace` (null in production): on the launch's last step every activation image and every gradient image,
//     as the backward read them, plus the fp32 logits and logit gradients, are copied out.
//
// Numerics = the bf16 layerwise TrainStep of this framework; tests/test_mlp_step_gpu.py checks every stage
// against fp64 from the kernel's own stored tensors.
#include <cstdint>

#include "common.h"
#include "optim_core.h"
#include "ops_api.h"
#include "wg_prims.h"

namespace mlps {
using namespace wgp;

constexpr int NT = 512, NW = NT / 64;
constexpr int MAXL = 8, MAXD = 64, MAXB = 64;
constexpr int XPT = MAXB * MAXD / NT;     // batch elements a thread stages
constexpr int LDS_MAX = 160 * 1024;
constexpr int TRACE_IMG = MAXB * MAXD;    // trace: [2 MAXL] dense 64 x 64 bf16 images, then z[64], g[64] fp32
constexpr int TRACE_ELEMS = 2 * MAXL * TRACE_IMG + 4 * MAXB;
// fp32 scratch arrays (float offsets in the fp32 region): hidden biases, last-layer weights (bf16-rounded)
// and bias, per-row logit gradient / logit / loss / hit, the labels (double-buffered)
constexpr int F_BIAS = 0, F_WL = F_BIAS + MAXL * MAXD, F_BL = F_WL + MAXD, F_GV = F_BL + 16, F_ZV = F_GV + MAXB,
              F_LR = F_ZV + MAXB, F_CR = F_LR + MAXB, F_Y = F_CR + MAXB, F_END = F_Y + 2 * MAXB;

// layer l: in -> out, act of its output (0 none, 1 relu, 2 sigmoid); input image A_l at offA (stride S,
// bf16 elements), weight image [16 OT][S] at offW; IT / OT = 16-wide input / output tiles; woff / boff =
// arena offsets of weight [out][in] and bias relative to the span start
struct Ly {
  int in, out, act, S, offA, offW, woff, boff, IT, OT;
};
struct Args {
  float* master;
  bf16_raw* shadow;
  float* m;
  float* v;
  const float* xs;
  const float* ys;
  long long* cursor;   // batch of the first step (advanced by nsteps), or null
  float* loss;         // [nsteps]
  int* correct;        // [nsteps]
  float* step_count;   // completed optimizer steps (advanced by nsteps)
  const float* hp_dev; // the optimizer's device hyper-parameter vector, or null
  bf16_raw* trace;     // [TRACE_ELEMS] or null
  OptHP hp;
  long lo;             // arena span [lo, lo + span)
  int span, L, B, nbatch, nsteps, kind, mse, ntile, R, lds_state;
  int offG[2], offF, offS, bytes;  // G images (bf16 elements); fp32 region / state copy (bytes); LDS bytes
  Ly ly[MAXL];
};

typedef const __attribute__((address_space(4))) Args* kargs_t;
// the arguments are read where used through the kernarg pointer (scalar loads with a runtime layer index;
// a by-value copy indexed at run time would live in scratch)
__device__ __forceinline__ kargs_t kargs() { return (kargs_t)__builtin_amdgcn_kernarg_segment_ptr(); }
__device__ __forceinline__ Ly ly_at(int l) {
  kargs_t p = kargs();
  Ly y;
  y.in = p->ly[l].in, y.out = p->ly[l].out, y.act = p->ly[l].act, y.S = p->ly[l].S, y.offA = p->ly[l].offA;
  y.offW = p->ly[l].offW, y.woff = p->ly[l].woff, y.boff = p->ly[l].boff, y.IT = p->ly[l].IT, y.OT = p->ly[l].OT;
  return y;
}

__device__ __forceinline__ float rbf(float f) { return b2f((short)f2bf_hw(f)); }
// operand with K along the row: lane l takes row r0 + (l & 15), 8 (or 4) consecutive k
__device__ __forceinline__ bf16x8 rd8(const bf16_raw* img, int S, int r0, int k0, int lane) {
  return *(const bf16x8*)(img + (r0 + (lane & 15)) * S + k0 + 8 * (lane >> 4));
}
__device__ __forceinline__ bf16x4 rd4(const bf16_raw* img, int S, int r0, int k0, int lane) {
  return *(const bf16x4*)(img + (r0 + (lane & 15)) * S + k0 + 4 * (lane >> 4));
}
// operand with K down the rows (transposed read): lane l gets column c0 + (l & 15) of rows k0 + 4 (l >> 4) + j
// (x16) or k0 + 8 (l >> 4) + j (x32).  EXEC must be full: only under wave-uniform branches.
__device__ __forceinline__ bf16x4 tr4(const bf16_raw* img, int S, int k0, int c0, int lane) {
  const int i = lane & 15;
  return lds_tr4(img + (k0 + 4 * (lane >> 4) + (i >> 2)) * S + c0 + 4 * (i & 3));
}
__device__ __forceinline__ bf16x8 tr8(const bf16_raw* img, int S, int k0, int c0, int lane) {
  const int i = lane & 15;
  const bf16_raw* p = img + (k0 + 8 * (lane >> 4) + (i >> 2)) * S + c0 + 4 * (i & 3);
  return lds_tr(p, p + 4 * S);
}
__device__ __forceinline__ void st4(bf16_raw* p, float a, float b, float c, float d) {
  *(bf16x4*)p = (bf16x4){(short)f2bf_hw(a), (short)f2bf_hw(b), (short)f2bf_hw(c), (short)f2bf_hw(d)};
}
// keeps the compiler from moving LDS accesses across it (this wave's own write -> read order)
__device__ __forceinline__ void fence_c() { asm volatile("" ::: "memory"); }

__device__ __forceinline__ float act_f(float z, int act) {
  return act == 1 ? fmaxf(z, 0.f) : act == 2 ? 1.f / (1.f + expf(-z)) : z;
}
// the activation's derivative from its (bf16) output
__device__ __forceinline__ float dact(float a, int act) {
  return act == 1 ? (a > 0.f ? 1.f : 0.f) : act == 2 ? a * (1.f - a) : 1.f;
}

// ---- forward of layer y for batch tile b0: A_{l+1}[b][o] = act(sum_k W[o][k] A_l[b][k] + bias[o]); rows >= B
// and columns >= out are written as zeros
__device__ __forceinline__ void fwd_tile(const bf16_raw* Lb, const float* bias, const Ly& y, const bf16_raw* Ain,
                                         bf16_raw* Aout, int So, int b0, int B, int lane) {
  const int b = b0 + (lane & 15), K = 16 * y.IT;
  const bf16_raw* W = Lb + y.offW;
  for (int ot = 0; ot < y.OT; ++ot) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int k = 0;
    for (; k + 32 <= K; k += 32) acc = mma32(rd8(W, y.S, 16 * ot, k, lane), rd8(Ain, y.S, b0, k, lane), acc);
    if (k < K) acc = mma16(rd4(W, y.S, 16 * ot, k, lane), rd4(Ain, y.S, b0, k, lane), acc);
    const int o = 16 * ot + 4 * (lane >> 4);
    const f32x4 bv = *(const f32x4*)(bias + o);
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = (b < B && o + r < y.out) ? act_f(acc[r] + bv[r], y.act) : 0.f;
    st4(Aout + b * So + o, v[0], v[1], v[2], v[3]);
  }
}

// ---- dX of layer y (k >= 1) for batch tile b0: G_{k-1}[b][i] = act'_{k-1}(A_k[b][i]) sum_o G_k[b][o] W_k[o][i]
// (columns i >= in: the image's W columns are zero)
__device__ __forceinline__ void dx_tile(const bf16_raw* Lb, const Ly& y, int actp, const bf16_raw* G, int SG,
                                        bf16_raw* Gout, int b0, int lane) {
  const int b = b0 + (lane & 15), K = 16 * y.OT;
  const bf16_raw* W = Lb + y.offW;
  for (int it = 0; it < y.IT; ++it) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int k = 0;
    for (; k + 32 <= K; k += 32) acc = mma32(tr8(W, y.S, k, 16 * it, lane), rd8(G, SG, b0, k, lane), acc);
    if (k < K) acc = mma16(tr4(W, y.S, k, 16 * it, lane), rd4(G, SG, b0, k, lane), acc);
    const int i = 16 * it + 4 * (lane >> 4);
    const bf16x4 av = *(const bf16x4*)(Lb + y.offA + b * y.S + i);
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = acc[r] * dact(b2f(av[r]), actp);
    st4(Gout + b * y.S + i, v[0], v[1], v[2], v[3]);
  }
}

// ---- the optimizer state of the launch: LDS copies of the arena span or the arena itself (generic pointers)
struct State {
  float *w, *m, *v;
  bf16_raw* sh;  // the arena's bf16 shadow at the span start (written on the launch's last step), or null
  OptHP h;
  float bc1, bc2;
  int kind;
  bool last;
};
__device__ __forceinline__ float adam_at(const State& s, int idx, float g) {
  float w = s.w[idx], m = s.m[idx], v = s.v[idx], s3 = 0.f;
  w = s.kind == 2 ? upd<2>(w, g * s.h.gscale, m, v, s3, s.h, s.bc1, s.bc2)
                  : upd<1>(w, g * s.h.gscale, m, v, s3, s.h, s.bc1, s.bc2);
  s.w[idx] = w;
  s.m[idx] = m;
  s.v[idx] = v;
  if (s.last && s.sh) s.sh[idx] = f2bf_hw(w);
  return w;
}

// dW tiles of layer y: t < IT OT the weight tile (i-tile t / OT, o-tile t % OT; accumulator element r of a lane:
// i = i0 + 4 (lane >> 4) + r, o = o0 + (lane & 15)), then OT bias tiles (lanes 0..15, element 0: o = o0 + lane).
// Tile t belongs to wave (t + first) % NW for the whole launch.
__device__ __forceinline__ void dw_tile(const bf16_raw* Lb, float* bias, const Ly& y, const bf16_raw* Ain,
                                        const bf16_raw* G, int SG, int t, int ntile, int lane, const State& s) {
  const int nwt = y.IT * y.OT;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (t < nwt) {
    const int i0 = 16 * (t / y.OT), o0 = 16 * (t % y.OT);
    for (int kt = 0; kt < ntile; ++kt) acc = mma16(tr4(Ain, y.S, 16 * kt, i0, lane), tr4(G, SG, 16 * kt, o0, lane), acc);
    const int i = i0 + 4 * (lane >> 4), o = o0 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (o < y.out && i + r < y.in) adam_at(s, y.woff + o * y.in + i + r, acc[r]);
  } else {
    const int o0 = 16 * (t - nwt);
    const short one = (short)0x3F80;  // bf16 1.0
    const bf16x4 ones = {one, one, one, one};
    for (int kt = 0; kt < ntile; ++kt) acc = mma16(ones, tr4(G, SG, 16 * kt, o0, lane), acc);
    const int o = o0 + lane;
    if (lane < 16 && o < y.out) bias[o] = adam_at(s, y.boff + o, acc[0]);
  }
}
// the bf16 image of weight tile t from the owner's fp32 weights (padding stays zero)
__device__ __forceinline__ void put_tile(bf16_raw* Lb, const Ly& y, int t, int lane, const float* w) {
  const int i = 16 * (t / y.OT) + 4 * (lane >> 4), o = 16 * (t % y.OT) + (lane & 15);
  float v[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = (o < y.out && i + r < y.in) ? w[y.woff + o * y.in + i + r] : 0.f;
  st4(Lb + y.offW + o * y.S + i, v[0], v[1], v[2], v[3]);
}

// dst[0..n) = src[0..n) (global -> LDS), 8 loads of a thread in flight at once; 16-byte loads when aligned
__device__ __forceinline__ void gather_in(float* dst, const float* src, int n, int tid) {
  constexpr int PER = 8;
  const int n4 = (((uintptr_t)src & 15) == 0) ? n >> 2 : 0;
  for (int base = 0; base < n4; base += NT * PER) {
    f32x4 v[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int e = base + tid + NT * k;
      v[k] = ((const f32x4*)src)[e < n4 ? e : 0];
    }
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (base + tid + NT * k < n4) ((f32x4*)dst)[base + tid + NT * k] = v[k];
  }
  for (int e = 4 * n4 + tid; e < n; e += NT) dst[e] = src[e];
}
__device__ __forceinline__ void scatter_out(float* dst, const float* src, int n, int tid) {
  const int n4 = (((uintptr_t)dst & 15) == 0) ? n >> 2 : 0;
  for (int e = tid; e < n4; e += NT) ((f32x4*)dst)[e] = ((const f32x4*)src)[e];
  for (int e = 4 * n4 + tid; e < n; e += NT) dst[e] = src[e];
}

// (trace) a dense [64][64] copy of the image's rows < R and its C (16 per tile) operand columns; zeros elsewhere.
// (The two G buffers serve layers of different strides: beyond a G's operand columns lie stale entries of other
// layers' images, which no product reads.)
__device__ __forceinline__ void trace_img(bf16_raw* dst, const bf16_raw* img, int S, int C, int R, int tid) {
  for (int e = tid; e < TRACE_IMG; e += NT) {
    const int r = e >> 6, c = e & 63;
    dst[e] = (r < R && c < C) ? img[r * S + c] : (bf16_raw)0;
  }
}

__global__ __launch_bounds__(NT) void mlp_step_k(Args A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  bf16_raw* const Lb = (bf16_raw*)lds;
  float* const LF = (float*)(lds + A.offF);
  const kargs_t C = kargs();
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = A.L, B = A.B, ntile = A.ntile, R = A.R;
  const bool tw = wave < ntile;          // tile wave
  const int b0 = 16 * wave;
  const int first = (wave + NW - ntile) & (NW - 1);  // this wave's first dW tile: waves without a batch tile lead
  const int S0 = A.ly[0].S, F = A.ly[0].in;

  State st;
  st.h = load_hp(A.hp, A.hp_dev);
  st.kind = A.kind;
  st.sh = A.shadow ? A.shadow + A.lo : nullptr;
  st.last = false;
  // ------------------------------------------------------------------ launch prologue
  {
    uint4* z = (uint4*)lds;
    const int nz = (A.lds_state ? A.offS : A.bytes) / 16;
    for (int e = tid; e < nz; e += NT) z[e] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (A.lds_state) {
    float* S = (float*)(lds + A.offS);
    const int sp = (A.span + 3) & ~3;  // (each copy 16-byte aligned in LDS: gather_in / scatter_out move f32x4)
    st.w = S, st.m = S + sp, st.v = S + 2 * sp;
    gather_in(st.w, A.master + A.lo, A.span, tid);
    gather_in(st.m, A.m + A.lo, A.span, tid);
    gather_in(st.v, A.v + A.lo, A.span, tid);
  } else {
    st.w = A.master + A.lo, st.m = A.m + A.lo, st.v = A.v + A.lo;
  }
  __syncthreads();
  // the images and fp32 biases from the fp32 weights
  for (int l = 0; l < L; ++l) {
    const Ly y = ly_at(l);
    if (l + 1 < L) {
      for (int e = tid; e < y.in * y.out; e += NT) {
        const int o = e / y.in, i = e - o * y.in;
        Lb[y.offW + o * y.S + i] = f2bf_hw(st.w[y.woff + e]);
      }
      if (tid < y.out) LF[F_BIAS + MAXD * l + tid] = st.w[y.boff + tid];
    } else {
      if (tid < y.in) LF[F_WL + tid] = rbf(st.w[y.woff + tid]);
      if (tid == 0) LF[F_BL] = st.w[y.boff];
    }
  }
  // the batch: thread -> elements e = tid + NT j of [B][F], image offset row S0 + column
  const long long bi0 = A.cursor ? A.cursor[0] % A.nbatch : 0;
  int bnx = (int)bi0;
  int xo[XPT];
  float nx[XPT], ny = 0.f;
#pragma unroll
  for (int j = 0; j < XPT; ++j) {
    const int e = tid + NT * j, r = e / F;
    xo[j] = e < B * F ? r * S0 + (e - r * F) : -1;
  }
  auto fetch = [&]() {
    const float* xb = C->xs + (long)bnx * (B * F);
#pragma unroll
    for (int j = 0; j < XPT; ++j) nx[j] = xo[j] >= 0 ? xb[tid + NT * j] : 0.f;
    ny = tid < B ? C->ys[(long)bnx * B + tid] : 0.f;
  };
  auto stage = [&](int buf) {
    bf16_raw* A0 = Lb + A.ly[0].offA + buf * R * S0;
#pragma unroll
    for (int j = 0; j < XPT; ++j)
      if (xo[j] >= 0) A0[xo[j]] = f2bf_hw(nx[j]);
    if (tid < B) LF[F_Y + MAXB * buf + tid] = ny;
  };
  fetch();
  stage(0);
  const float t0 = A.step_count ? A.step_count[0] : 0.f;
  const float invB = 1.f / (float)B;
  bar();

  for (int step = 0; step < A.nsteps; ++step) {
    const int cur = step & 1;
    st.last = step + 1 == A.nsteps;
    const bool tr = st.last && A.trace != nullptr;
    bias_corr<1>(st.h, t0 + (float)(step + 1), st.bc1, st.bc2);
    const bf16_raw* A0 = Lb + A.ly[0].offA + cur * R * S0;
    if (!st.last) {  // the next batch, in flight during the step
      bnx = bnx + 1 == A.nbatch ? 0 : bnx + 1;
      fetch();
    }
    // ============================================================ FWD: tile waves, no barrier inside
    if (tw) {
      const bf16_raw* Ain = A0;
      for (int l = 0; l + 1 < L; ++l) {
        const Ly y = ly_at(l);
        const int offO = C->ly[l + 1].offA, So = C->ly[l + 1].S;
        fwd_tile(Lb, LF + F_BIAS + MAXD * l, y, Ain, Lb + offO, So, b0, B, lane);
        fence_c();
        Ain = Lb + offO;
      }
      // the last layer: z = a . w + b over the image's 16-column groups, folded over the 4 lane groups
      const Ly yl = ly_at(L - 1);
      const int q = lane >> 4, b = b0 + (lane & 15);
      float zd = 0.f;
      if (q < yl.IT) {
        const bf16x8 a0 = *(const bf16x8*)(Ain + b * yl.S + 16 * q), a1 = *(const bf16x8*)(Ain + b * yl.S + 16 * q + 8);
#pragma unroll
        for (int c = 0; c < 8; ++c) zd = fmaf(b2f(a0[c]), LF[F_WL + 16 * q + c], zd);
#pragma unroll
        for (int c = 0; c < 8; ++c) zd = fmaf(b2f(a1[c]), LF[F_WL + 16 * q + 8 + c], zd);
      }
      zd += __shfl_xor(zd, 16, 64);
      zd += __shfl_xor(zd, 32, 64);
      const float z = zd + LF[F_BL], yv = LF[F_Y + MAXB * cur + b];
      const bool vb = b < B;
      float g, ls, hit = 0.f;
      if (A.mse) {
        const float d = z - yv;
        g = 2.f * d * invB;
        ls = d * d;
      } else {
        const float e = expf(-fabsf(z));
        const float p = z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        g = (p - yv) * invB;
        ls = fmaxf(z, 0.f) - z * yv + log1pf(e);
        hit = (float)((z > 0.f) == (yv > 0.5f));
      }
      g = vb ? g : 0.f;
      if (q == 0) {
        LF[F_GV + b] = g;
        LF[F_ZV + b] = z;
        LF[F_LR + b] = vb ? ls : 0.f;
        LF[F_CR + b] = vb ? hit : 0.f;
      }
      if (L >= 2) {  // G_{L-2}[b][o] = g w[o] act'(a[b][o]) (w is zero beyond the width)
        const int actp = C->ly[L - 2].act;
        bf16_raw* G = Lb + A.offG[(L - 2) & 1];
        for (int ot = 0; ot < yl.IT; ++ot) {
          const int o = 16 * ot + 4 * q;
          const bf16x4 av = *(const bf16x4*)(Ain + b * yl.S + o);
          const f32x4 w4 = *(const f32x4*)(LF + F_WL + o);
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = g * w4[r] * dact(b2f(av[r]), actp);
          st4(G + b * yl.S + o, v[0], v[1], v[2], v[3]);
        }
      }
    }
    bar();
    if (tr) {
      for (int l = 0; l < L; ++l)
        trace_img(A.trace + l * TRACE_IMG, l ? Lb + C->ly[l].offA : A0, C->ly[l].S, 16 * C->ly[l].IT, R, tid);
      float* tf = (float*)(A.trace + 2 * MAXL * TRACE_IMG);
      if (tid < MAXB) {
        tf[tid] = tid < R ? LF[F_ZV + tid] : 0.f;
        tf[MAXB + tid] = tid < R ? LF[F_GV + tid] : 0.f;
      }
    }
    // ============================================================ the last layer (wave 7, in the first backward
    // phase): the step's loss / hits (fixed shuffle tree), its gradients in example order, Adam, new fp32 copies
    auto last_layer = [&]() {
      const Ly yl = ly_at(L - 1);
      const bf16_raw* Al = L == 1 ? A0 : Lb + yl.offA;
      const float lsum = wave_sum(lane < B ? LF[F_LR + lane] : 0.f), csum = wave_sum(lane < B ? LF[F_CR + lane] : 0.f);
      if (lane == 0) {
        if (A.loss) A.loss[step] = lsum * invB;
        if (A.correct) A.correct[step] = (int)csum;
      }
      if (lane < yl.in) {
        float g = 0.f;
        for (int b = 0; b < B; ++b) g = fmaf(LF[F_GV + b], b2f((short)Al[b * yl.S + lane]), g);
        LF[F_WL + lane] = rbf(adam_at(st, yl.woff + lane, g));
      }
      if (lane == 0) {
        float g = 0.f;
        for (int b = 0; b < B; ++b) g += LF[F_GV + b];
        LF[F_BL] = adam_at(st, yl.boff, g);
      }
    };
    if (L == 1) {  // no hidden layer: the last layer is the whole backward
      if (wave == NW - 1) last_layer();
      if (!st.last) stage(cur ^ 1);
      bar();
    }
    // ============================================================ backward phases k = L-2 .. 0: tile waves dX_k ;
    // every wave: W_{k+1}'s new image (its dX ran one phase earlier), its dW_k tiles + Adam (k = 0: W_0's image too)
    for (int k = L - 2; k >= 0; --k) {
      if (k == L - 2 && wave == NW - 1) last_layer();
      const Ly y = ly_at(k);
      const int SG = C->ly[k + 1].S;  // G_k's stride: that of A_{k+1}
      const bf16_raw* G = Lb + A.offG[k & 1];
      if (tr) trace_img(A.trace + (MAXL + k) * TRACE_IMG, G, SG, 16 * y.OT, R, tid);
      if (tw && k >= 1) dx_tile(Lb, y, C->ly[k - 1].act, G, SG, Lb + A.offG[(k - 1) & 1], b0, lane);
      if (k + 2 < L) {
        const Ly yn = ly_at(k + 1);
        for (int t = first; t < yn.IT * yn.OT; t += NW) put_tile(Lb, yn, t, lane, st.w);
      }
      const bf16_raw* Ain = k ? Lb + y.offA : A0;
      const int nt = y.IT * y.OT + y.OT;
      for (int t = first; t < nt; t += NW) dw_tile(Lb, LF + F_BIAS + MAXD * k, y, Ain, G, SG, t, ntile, lane, st);
      if (k == 0) {
        fence_c();
        for (int t = first; t < y.IT * y.OT; t += NW) put_tile(Lb, y, t, lane, st.w);
        if (!st.last) stage(cur ^ 1);
      }
      bar();
    }
  }

  // ------------------------------------------------------------------ write-back
  __syncthreads();
  if (A.lds_state) {
    scatter_out(A.master + A.lo, st.w, A.span, tid);
    scatter_out(A.m + A.lo, st.m, A.span, tid);
    scatter_out(A.v + A.lo, st.v, A.span, tid);
  }
  if (tid == 0) {
    if (A.step_count) A.step_count[0] = t0 + (float)A.nsteps;
    if (A.cursor) A.cursor[0] = (bi0 + A.nsteps) % A.nbatch;
  }
}

constexpr int pad16(int x) { return (x + 15) & ~15; }
// row stride of an image of `w` columns: the smallest odd multiple of 16 elements that holds them
constexpr int stride_of(int w) { return pad16(w) / 16 % 2 ? pad16(w) : pad16(w) + 16; }

// iv: L B nbatch nsteps kind(1 adam, 2 adamw) loss(0 bce_logits, 1 mse) dims[L+1] acts[L] woff[L] boff[L]
// (arena offsets; a layer without a bias: -1).  0 = this kernel takes the configuration.
int fill(Args& a, const long* iv, int ni) {
  if (ni < 6) return -1;
  const int L = (int)iv[0];
  if (L < 1 || L > MAXL || ni != 6 + (L + 1) + 3 * L) return -1;
  a.L = L, a.B = (int)iv[1], a.nbatch = (int)iv[2], a.nsteps = (int)iv[3], a.kind = (int)iv[4], a.mse = (int)iv[5];
  if (a.B < 1 || a.B > MAXB || a.nbatch < 1 || a.nsteps < 1 || (a.kind != 1 && a.kind != 2) || (a.mse != 0 && a.mse != 1))
    return -1;
  const long *dims = iv + 6, *acts = dims + L + 1, *woff = acts + L, *boff = woff + L;
  for (int i = 0; i <= L; ++i)
    if (dims[i] < 1 || dims[i] > MAXD) return -1;
  if (dims[L] != 1 || acts[L - 1] != 0) return -1;
  long lo = woff[0], hi = woff[0];
  for (int l = 0; l < L; ++l) {
    if (acts[l] < 0 || acts[l] > 2 || woff[l] < 0 || boff[l] < 0) return -1;
    const long we = woff[l] + dims[l] * dims[l + 1], be = boff[l] + dims[l + 1];
    lo = woff[l] < lo ? woff[l] : lo;
    lo = boff[l] < lo ? boff[l] : lo;
    hi = we > hi ? we : hi;
    hi = be > hi ? be : hi;
  }
  // (a span of this size is a model of these widths with its 64-element alignment gaps, nothing else)
  if (hi - lo > 2L * MAXL * (MAXD * MAXD + 2 * MAXD)) return -1;
  a.lo = lo, a.span = (int)(hi - lo);
  a.ntile = (a.B + 15) / 16, a.R = 16 * a.ntile;
  int off = 0, smax = 16;
  for (int l = 0; l < L; ++l) {
    Ly& y = a.ly[l];
    y.in = (int)dims[l], y.out = (int)dims[l + 1], y.act = (int)acts[l], y.S = stride_of(y.in);
    y.IT = pad16(y.in) / 16, y.OT = pad16(y.out) / 16;
    y.woff = (int)(woff[l] - lo), y.boff = (int)(boff[l] - lo);
    y.offA = off;
    off += (l ? 1 : 2) * a.R * y.S;  // (the input image is double-buffered)
    if (l) smax = y.S > smax ? y.S : smax;
  }
  for (int g = 0; g < 2; ++g) {
    a.offG[g] = off;
    off += L >= 2 ? a.R * smax : 0;
  }
  for (int l = 0; l + 1 < L; ++l) {
    a.ly[l].offW = off;
    off += 16 * a.ly[l].OT * a.ly[l].S;
  }
  a.ly[L - 1].offW = 0;
  a.offF = (2 * off + 15) & ~15;
  a.offS = a.offF + 4 * F_END;
  const long with_state = (long)a.offS + 12L * ((a.span + 3) & ~3);  // (three 16-byte aligned copies)
  a.lds_state = with_state <= LDS_MAX;
  a.bytes = a.lds_state ? (int)with_state : a.offS;
  return a.bytes <= LDS_MAX ? 0 : -1;
}

}  // namespace mlps

// The LDS bytes of the launch if the kernel takes this configuration (iv as hopsx_mlp_step's), else -1.
extern "C" long hopsx_mlp_step_ok(const long* iv, int ni) {
  mlps::Args a{};
  return mlps::fill(a, iv, ni) ? -1 : a.bytes;
}
// g: LDS bytes, optimizer state in LDS (1) or updated in place in the arena (0), batch tiles, trace elements
// (bf16), trace image elements.  Returns 0, or -1 for a configuration the kernel does not take.
extern "C" int hopsx_mlp_step_geom(const long* iv, int ni, long* g) {
  mlps::Args a{};
  if (mlps::fill(a, iv, ni)) return -1;
  g[0] = a.bytes, g[1] = a.lds_state, g[2] = a.ntile, g[3] = mlps::TRACE_ELEMS, g[4] = mlps::TRACE_IMG;
  return 0;
}

// ptrs: master shadow adam_m adam_v xs ys cursor loss correct step_count hp_dev trace (0 = none, from cursor on;
// shadow may be 0 too).  fv: the optimizer's 8 hyper-parameters (used when hp_dev is 0).
extern "C" int hopsx_mlp_step(const uint64_t* p, int np, const long* iv, int ni, const float* fv, int nf,
                              hipStream_t st) {
  mlps::Args a{};
  if (np != 12 || nf != 8 || mlps::fill(a, iv, ni)) return -2;
  a.master = (float*)p[0];
  a.shadow = (bf16_raw*)p[1];
  a.m = (float*)p[2];
  a.v = (float*)p[3];
  a.xs = (const float*)p[4];
  a.ys = (const float*)p[5];
  a.cursor = (long long*)p[6];
  a.loss = (float*)p[7];
  a.correct = (int*)p[8];
  a.step_count = (float*)p[9];
  a.hp_dev = (const float*)p[10];
  a.trace = (bf16_raw*)p[11];
  if (!a.master || !a.m || !a.v || !a.xs || !a.ys) return -2;
  if (!a.cursor && a.nbatch != 1) return -2;
  a.hp = OptHP{fv[0], fv[1], fv[2], fv[3], fv[4], fv[5], fv[6], fv[7]};
  static bool attr = false;
  if (!attr) {
    const hipError_t e = hipFuncSetAttribute((const void*)mlps::mlp_step_k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             mlps::LDS_MAX);
    if (e != hipSuccess) return (int)e;
    attr = true;
  }
  hipLaunchKernelGGL(mlps::mlp_step_k, dim3(1), dim3(mlps::NT), (size_t)a.bytes, st, a);
  return (int)hipGetLastError();
}
