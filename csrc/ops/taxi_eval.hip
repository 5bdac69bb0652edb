// hopsx: forward-only evaluation of the Chicago-taxi wide & deep model over N resident rows in ONE launch
// (gfx950), with per-row outputs and TFMA-style overall / per-slice metric accumulators.
//
// Model: models/widedeep.py (dense 3 -> 100 -> 70 -> 48 -> 34 -> 1, relu on the four hidden layers, plus the
// sum of 13 rows of the 6,287-row wide table); the training side is taxi_step.hip.
//
// Partition: by 16-row MFMA tile.  One wave owns a tile and runs its whole forward (four hidden layers, the
// logit, the loss) with no workgroup barrier, as the "tile waves" of taxi_step.hip do.  A workgroup of 256
// threads takes four tiles per trip and walks the tiles in a grid-stride loop; nothing crosses workgroups
// except integer atomics on the accumulators: no hand-off, no flag, no co-residency requirement.
//
// Once per workgroup the four hidden weight matrices are staged into LDS as bf16 images from the arena's bf16
// shadow; the biases, the logits weights w4 and the wide table (25 KB) are staged in fp32 from the master.
// A layer computes Z^T[o][b] = sum_k W[o][k] A[b][k] (`v_mfma_f32_16x16x32_bf16`, and one `16x16x16` for the
// odd last 16 inputs), so a lane ends up with 4 consecutive outputs o = 16 t + 4 g + r of ITS row b: exactly
// the 4 values the 16x16x16 B operand wants from it, and two such tiles are what the 16x16x32 B operand wants
// if k-slot 32 kk + 8 g + j stands for input 16 (2 kk + j / 4) + 4 g + j % 4.  The W images are staged in that
// k order, so the activations never leave the registers.  Image row strides are odd multiples of 16 elements
// (the training kernel's rule).  The next trip's 120 bytes per row (3 floats, 13 int64 ids, 1 float label)
// are requested before the current trip's MFMAs and stay in flight under them: the kernel is bound by that
// stream, not by its ~12 k MACs per row.
//
// Numerics: the rounding points of the v2 training kernel's forward (inputs and the four hidden activations
// rounded to bf16, bf16 W images, fp32 accumulation, fp32 biases in the epilogue; the logits layer an fp32
// dot product with the fp32 w4, plus b4, plus the 13 wide rows in column order 0..12; p = sigmoid(z); loss =
// max(z, 0) - z y + log1p(exp(-|z|)) with y = label > 0.5).
//
// Contract: a row's outputs depend only on that row and the weights (bit-identical for any n, any position
// in the set and any grid size); tail rows of the last tile are computed from zeros, never loaded past the
// inputs' ends, never stored and never counted.  Every accumulator is an integer (histogram counts, hit
// counts, 2^-24 fixed-point sums of loss and probability), so the result does not depend on atomic order
// or grid size.  A wide id outside [0, rows) adds nothing to the logit, a slice id outside its column's range
// leaves the row out of every slice (still in "overall"); both are reported through hx_guard.  The launch
// path allocates nothing, synchronises nothing and issues no memset (the accumulators are cleared by a
// kernel of this file): capture-safe.
#include "common.h"
#include "taxi_wd.h"
#include "wg_prims.h"

namespace taxiev {
// Shared with the training kernel by construction, not by comment: the device vocabulary (f2bf_hw, b2f,
// the held MFMA forms) and the model geometry (NWIDE, D0..D4, the wide columns' cardinalities CARD, cdiv,
// the fp32 bias / w4 map F_B0..F_W4 that both kernels stage the same way).  The W images, the LDS map,
// the tile size and Args below are this kernel's own.
using namespace wgp;
using namespace taxi_wd;

constexpr int NT = 256;      // 4 waves, one 16-row tile each per trip
constexpr int TR = 16;       // rows per tile
constexpr int WROWS = 6288;  // wide rows the LDS table holds (the model has 6,287)
constexpr int NB = 1024;     // probability bins
constexpr int SMAX = 128;    // slices
constexpr float QSCALE = 16777216.f;  // 2^24 fixed point of the loss / probability sums

// rows of the model's wide table: the 13 columns back to back
constexpr int wide_rows() {
  int t = 0;
  for (int c = 0; c < NWIDE; ++c) t += CARD[c];
  return t;
}
static_assert(wide_rows() == 6287 && wide_rows() <= WROWS, "the LDS wide table holds the model's rows");
// columns that may be the slice column: at most SMAX values (not the vocabularies and census tracts); a
// row's slice is its value in that column
constexpr bool sliceable(int c) { return CARD[c] <= SMAX; }


// layer: IN -> OUT.  IT input tiles of 16 (NK32 pairs for the x32 MFMA + one x16 tail), OT output tiles;
// W image [16 OT][K] bf16 at byte offset LW, fp32 bias [16 OT] at float offset FB (both zero beyond OUT / IN)
template <int IN_, int OUT_, int LW_, int FB_>
struct Layer {
  static constexpr int IN = IN_, OUT = OUT_, LW = LW_, FB = FB_;
  static constexpr int IT = cdiv(IN_, 16), OT = cdiv(OUT_, 16), NK32 = IT / 2, K = 16 * IT;
  static constexpr int BYTES = 16 * OT * K * 2;
  static_assert(IT % 2 == 1, "row stride: an odd multiple of 16 elements (and one x16 tail tile)");
  // the input feature at k-slot pos of the image
  __host__ __device__ static constexpr int feat(int pos) {
    return pos < 32 * NK32 ? 16 * (2 * (pos >> 5) + ((pos & 7) >> 2)) + 4 * ((pos & 31) >> 3) + (pos & 3) : pos;
  }
};
constexpr int F_MISC = F_W4_END, F_END = F_MISC + 16;  // b4 behind taxi_wd.h's bias / w4 map
using L0 = Layer<D0, D1, 0, F_B0>;
using L1 = Layer<D1, D2, L0::LW + L0::BYTES, F_B1>;
using L2 = Layer<D2, D3, L1::LW + L1::BYTES, F_B2>;
using L3 = Layer<D3, D4, L2::LW + L2::BYTES, F_B3>;
static_assert(L1::IT == L0::OT && L2::IT == L1::OT && L3::IT == L2::OT, "a layer's input tiles are its producer's");
// taxi_wd.h's map is laid out in whole output tiles of these layers; w4 is read as one f32x4 per lane
// group and output tile of layer 3, so it spans L3's tiles too
static_assert(F_B1 - F_B0 == 16 * L0::OT && F_B2 - F_B1 == 16 * L1::OT && F_B3 - F_B2 == 16 * L2::OT &&
                  F_W4 - F_B3 == 16 * L3::OT && F_W4_END - F_W4 == 16 * L3::OT,
              "bias / w4 map: whole output tiles");

// LDS map (bytes, every offset a multiple of 16)
constexpr int L_F = L3::LW + L3::BYTES;            // f32  biases, w4, b4
constexpr int L_WT = L_F + F_END * 4;              // f32  [WROWS] wide table
constexpr int L_HIST = L_WT + WROWS * 4;           // u32  [2 label][NB] overall histogram of this workgroup
constexpr int L_SUM = L_HIST + 2 * NB * 4;         // u64  [1 + SMAX][3] hits, loss_q, prob_q of this workgroup
constexpr int LDS_BYTES = L_SUM + (1 + SMAX) * 3 * 8;
static_assert(L_F % 16 == 0 && L_WT % 16 == 0 && L_HIST % 16 == 0 && L_SUM % 16 == 0, "LDS alignment");
static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");

struct Args {
  const float* master;      // arena fp32 parameters
  const bf16_raw* shadow;   // arena bf16 copy (hidden weights)
  long woff[5], boff[5];    // arena offsets of the 5 Linear layers
  long wide_off;
  int rows;                 // wide table rows (<= WROWS)
  const float* dense;       // [n][3]
  const long long* cat;     // [n][13] global one-hot ids
  const float* label;       // [n] or null (logits / probabilities only)
  long n;
  long ntiles;
  float* logit;             // [n]
  float* prob;              // [n]
  float* loss;              // [n]
  unsigned char* hit;       // [n]
  unsigned long long* sums; // [1 + S][3] hits, loss_q, prob_q
  unsigned* hist;           // [1 + S][2 label][NB]
  int slice_col;            // -1: no slices
  int slice_card;           // S
  long long slice_lo;       // global id of the slice column's value 0
};

// MFMA: the activations of a row tile live in registers from layer to layer, across every MFMA, so this
// kernel uses wg_prims.h's HELD forms (mma32_held / mma16_held: the operands stay alive for 4 wait states
// after the issue).  Do not switch them to the plain forms: the products come out wrong.

// W image of layer Ly from the shadow's row-major [OUT][IN]: k-permuted, zero beyond OUT / IN.  Every load
// is issued before the first store (clamped addresses, masked values: no branch around a load)
template <class Ly>
__device__ __forceinline__ void stage_w(unsigned char* smem, const bf16_raw* src, int tid) {
  bf16_raw* img = (bf16_raw*)(smem + Ly::LW);
  if constexpr (Ly::IN % 2 == 0) {  // pairs (f, f + 1) sit at k-slots (pos, pos + 1): 4-byte loads
    constexpr int HP = Ly::K / 2, TOT = 16 * Ly::OT * HP, NQ = cdiv(TOT, NT);
    unsigned v[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int i = tid + NT * q, o = i / HP, f = Ly::feat(2 * (i - o * HP));
      const bool keep = o < Ly::OUT && f < Ly::IN;
      v[q] = *(const unsigned*)(src + (keep ? o * Ly::IN + f : 0));
      v[q] = keep ? v[q] : 0u;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int i = tid + NT * q, o = i / HP;
      if (i < TOT) *(unsigned*)(img + o * Ly::K + 2 * (i - o * HP)) = v[q];
    }
  } else {
    constexpr int TOT = 16 * Ly::OT * Ly::K, NQ = cdiv(TOT, NT);
    bf16_raw v[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int i = tid + NT * q, o = i / Ly::K, f = Ly::feat(i - o * Ly::K);
      const bool keep = o < Ly::OUT && f < Ly::IN;
      v[q] = src[keep ? o * Ly::IN + f : 0];
      v[q] = keep ? v[q] : (bf16_raw)0;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int i = tid + NT * q;
      if (i < TOT) img[i] = v[q];
    }
  }
}

// dst[0..cap) = src[0..n), zero beyond
template <int CAP>
__device__ __forceinline__ void stage_f(float* dst, const float* src, int n, int tid) {
  constexpr int NQ = cdiv(CAP, NT);
  float v[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = tid + NT * q;
    v[q] = src[i < n ? i : 0];
    v[q] = i < n ? v[q] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = tid + NT * q;
    if (i < CAP) dst[i] = v[q];
  }
}

// one layer of this wave's tile: in[IT] / out[OT] are the lane's 4 consecutive features of its row per tile
template <class Ly>
__device__ __forceinline__ void layer(const unsigned char* smem, const bf16x4* in, bf16x4* out, int lane) {
  const bf16_raw* W = (const bf16_raw*)(smem + Ly::LW);
  const float* bias = (const float*)(smem + L_F) + Ly::FB;
  const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
  for (int ot = 0; ot < Ly::OT; ++ot) {
    const bf16_raw* wrow = W + (16 * ot + fr) * Ly::K;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < Ly::NK32; ++kk) {
      const bf16x4 lo = in[2 * kk], hi = in[2 * kk + 1];
      const bf16x8 b = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      acc = mma32_held(*(const bf16x8*)(wrow + 32 * kk + 8 * fq), b, acc);
    }
    acc = mma16_held(*(const bf16x4*)(wrow + 32 * Ly::NK32 + 4 * fq), in[Ly::IT - 1], acc);
    const f32x4 bv = *(const f32x4*)(bias + 16 * ot + 4 * fq);
    out[ot] = (bf16x4){(short)f2bf_hw(fmaxf(acc[0] + bv[0], 0.f)), (short)f2bf_hw(fmaxf(acc[1] + bv[1], 0.f)),
                       (short)f2bf_hw(fmaxf(acc[2] + bv[2], 0.f)), (short)f2bf_hw(fmaxf(acc[3] + bv[3], 0.f))};
  }
}

// a lane's share of its row's 120 input bytes: lane (b = lane & 15, g = lane >> 4) takes the dense
// features and the label of row b and the ids of columns g, g + 4, g + 8, g + 12
struct RowIn {
  float x[3];
  long long id[4];
  float y;
};

__global__ __launch_bounds__(NT, 2) void taxi_eval_k(const Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, eb = lane & 15, eg = lane >> 4;
  float* LF = (float*)(smem + L_F);
  float* WT = (float*)(smem + L_WT);
  unsigned* HIST = (unsigned*)(smem + L_HIST);
  unsigned long long* SUM = (unsigned long long*)(smem + L_SUM);
  const bool labelled = a.label != nullptr;
  const int nsum = (1 + a.slice_card) * 3;

  // ---- parameters that stay in LDS for every tile of this workgroup ----
  stage_w<L0>(smem, a.shadow + a.woff[0], tid);
  stage_w<L1>(smem, a.shadow + a.woff[1], tid);
  stage_w<L2>(smem, a.shadow + a.woff[2], tid);
  stage_w<L3>(smem, a.shadow + a.woff[3], tid);
  stage_f<16 * L0::OT>(LF + F_B0, a.master + a.boff[0], D1, tid);
  stage_f<16 * L1::OT>(LF + F_B1, a.master + a.boff[1], D2, tid);
  stage_f<16 * L2::OT>(LF + F_B2, a.master + a.boff[2], D3, tid);
  stage_f<16 * L3::OT>(LF + F_B3, a.master + a.boff[3], D4, tid);
  stage_f<16 * L3::OT>(LF + F_W4, a.master + a.woff[4], D4, tid);
  stage_f<16>(LF + F_MISC, a.master + a.boff[4], 1, tid);
  stage_f<WROWS>(WT, a.master + a.wide_off, a.rows, tid);
  for (int i = tid; i < 2 * NB; i += NT) HIST[i] = 0u;
  for (int i = tid; i < (1 + SMAX) * 3; i += NT) SUM[i] = 0ull;
  __syncthreads();

  // clamped, branch-free loads of tile t's inputs (a tile or row past the end reads row 0 and is masked
  // where it is used)
  auto load = [&](long t, RowIn& in) {
    const long row = t * TR + eb;
    const long rc = t < a.ntiles && row < a.n ? row : 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) in.x[k] = a.dense[rc * D0 + k];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int c = eg + 4 * m;
      in.id[m] = a.cat[rc * NWIDE + (c < NWIDE ? c : NWIDE - 1)];
    }
    in.y = labelled ? a.label[rc] : 0.f;
  };

  unsigned long long hits = 0ull, lsum = 0ull, psum = 0ull;  // "overall", this lane's rows
  const long tstride = 4L * gridDim.x;
  long t = 4L * blockIdx.x + w;
  RowIn cur, nxt;
  load(t, cur);
#pragma unroll 1
  for (; t < a.ntiles; t += tstride) {
    load(t + tstride, nxt);  // in flight under this tile's MFMAs
    const long row = t * TR + eb;
    const bool live = row < a.n;  // rows past n: the tail, computed from zeros

    // ---- wide part: this lane's columns from the LDS table; the row's sum in column order 0..12 ----
    float wv[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int c = eg + 4 * m;
      bool ok = false;
      if (live && c < NWIDE) ok = hx_guard((unsigned long long)cur.id[m] < (unsigned long long)a.rows);
      const float v = WT[ok ? (int)cur.id[m] : 0];
      wv[m] = ok ? v : 0.f;
    }
    float ws = 0.f;
#pragma unroll
    for (int c = 0; c < NWIDE; ++c) ws += __shfl(wv[c >> 2], eb + 16 * (c & 3), 64);
    // the row's slice: computed by the lane that holds the slice column, -1 = in no slice
    int sl = -1;
    if (a.slice_col >= 0) {
      const int sm = a.slice_col >> 2;
      const long long idv = sm == 0 ? cur.id[0] : sm == 1 ? cur.id[1] : sm == 2 ? cur.id[2] : cur.id[3];
      const long long d = idv - a.slice_lo;
      if (live && eg == (a.slice_col & 3) && hx_guard(d >= 0 && d < (long long)a.slice_card)) sl = (int)d;
      sl = __shfl(sl, eb + 16 * (a.slice_col & 3), 64);
    }

    // ---- deep part ----
    bf16x4 a0 = {0, 0, 0, 0};
    if (live && eg == 0) a0 = (bf16x4){(short)f2bf_hw(cur.x[0]), (short)f2bf_hw(cur.x[1]), (short)f2bf_hw(cur.x[2]), 0};
    bf16x4 h1[L0::OT], h2[L1::OT], h3[L2::OT], h4[L3::OT];
    layer<L0>(smem, &a0, h1, lane);
    layer<L1>(smem, h1, h2, lane);
    layer<L2>(smem, h2, h3, lane);
    layer<L3>(smem, h3, h4, lane);
    // logit = a4 . w4 + b4 + the wide sum (w4 is zero beyond its 34 entries)
    float zd = 0.f;
#pragma unroll
    for (int ot = 0; ot < L3::OT; ++ot) {
      const f32x4 w4 = *(const f32x4*)(LF + F_W4 + 16 * ot + 4 * eg);
#pragma unroll
      for (int r = 0; r < 4; ++r) zd = fmaf(b2f(h4[ot][r]), w4[r], zd);
    }
    zd += __shfl_xor(zd, 16, 64);
    zd += __shfl_xor(zd, 32, 64);
    const float z = zd + LF[F_MISC] + ws;
    const float e = __expf(-fabsf(z));
    const float re = __builtin_amdgcn_rcpf(1.f + e);
    const float p = z >= 0.f ? re : e * re;

    if (live && eg == 0) {
      a.logit[row] = z;
      a.prob[row] = p;
      if (labelled) {
        const int y = cur.y > 0.5f ? 1 : 0;
        const float l = fmaxf(z, 0.f) - (y ? z : 0.f) + log1pf(e);
        const unsigned h = (unsigned)((z > 0.f) == (y != 0));
        a.loss[row] = l;
        a.hit[row] = (unsigned char)h;
        int bin = (int)(p * (float)NB);
        bin = bin < NB - 1 ? bin : NB - 1;
        bin = bin > 0 ? bin : 0;
        const unsigned long long lq = (unsigned long long)llrintf(l * QSCALE);
        const unsigned long long pq = (unsigned long long)llrintf(p * QSCALE);
        atomicAdd(&HIST[y * NB + bin], 1u);
        hits += h;
        lsum += lq;
        psum += pq;
        if (sl >= 0) {
          atomicAdd(&a.hist[((long)(1 + sl) * 2 + y) * NB + bin], 1u);
          atomicAdd(&SUM[(1 + sl) * 3 + 0], (unsigned long long)h);
          atomicAdd(&SUM[(1 + sl) * 3 + 1], lq);
          atomicAdd(&SUM[(1 + sl) * 3 + 2], pq);
        }
      }
    }
    cur = nxt;
  }

  // ---- flush this workgroup's integers ----
  if (labelled) {
    if (hits) atomicAdd(&SUM[0], hits);
    if (lsum) atomicAdd(&SUM[1], lsum);
    if (psum) atomicAdd(&SUM[2], psum);
    __syncthreads();
    for (int i = tid; i < 2 * NB; i += NT) {
      const unsigned v = HIST[i];
      if (v) atomicAdd(&a.hist[i], v);
    }
    for (int i = tid; i < nsum; i += NT) {
      const unsigned long long v = SUM[i];
      if (v) atomicAdd(&a.sums[i], v);
    }
  }
}

// the accumulators' clear: a kernel, so that a captured graph holds no memset node
__global__ __launch_bounds__(256) void taxi_eval_clear_k(unsigned long long* p, long n) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += 256L * gridDim.x) p[i] = 0ull;
}

}  // namespace taxiev

HOPSX_DBG_TU(taxi_eval)

// ptrs: master shadow dense cat label(0 = logits / probabilities only) logit prob loss hit acc
//       acc = uint64 [(1 + S) * 3] sums {hits, loss_q, prob_q} followed by uint32 [1 + S][2][NB] histograms
// iv:   woff[5] boff[5] wide_off rows n slice_col(-1 = none) max_workgroups(0 = 2 per CU)
extern "C" int hopsx_taxi_eval(const uint64_t* p, int np, const long* iv, int ni, hipStream_t st) {
  using namespace taxiev;
  if (np < 10 || ni < 15) return (int)hipErrorInvalidValue;
  const long rows = iv[11], n = iv[12], scol = iv[13];
  if (n < 0 || n >= 0x80000000L) return (int)hipErrorInvalidValue;  // the fixed-point sums' budget
  if (rows < 1 || rows > WROWS || scol < -1 || scol >= NWIDE) return (int)hipErrorInvalidValue;
  Args a{};
  a.slice_col = (int)scol;
  if (scol >= 0) {
    long lo = 0, total = 0;
    for (int c = 0; c < NWIDE; ++c) {
      if (c < scol) lo += CARD[c];
      total += CARD[c];
    }
    if (!sliceable(scol) || rows != total) return (int)hipErrorInvalidValue;  // vocabularies, census tracts
    a.slice_lo = lo;
    a.slice_card = CARD[scol];
  }
  if (n == 0) return (int)hipSuccess;
  a.master = (const float*)p[0];
  a.shadow = (const bf16_raw*)p[1];
  a.dense = (const float*)p[2];
  a.cat = (const long long*)p[3];
  a.label = (const float*)p[4];
  a.logit = (float*)p[5];
  a.prob = (float*)p[6];
  a.loss = (float*)p[7];
  a.hit = (unsigned char*)p[8];
  a.sums = (unsigned long long*)p[9];
  for (int k = 0; k < 5; ++k) {
    a.woff[k] = iv[k];
    a.boff[k] = iv[5 + k];
    if (a.woff[k] < 0 || a.boff[k] < 0) return (int)hipErrorInvalidValue;
  }
  a.wide_off = iv[10];
  a.rows = (int)rows;
  a.n = n;
  a.ntiles = (n + TR - 1) / TR;
  if (!a.master || !a.shadow || !a.dense || !a.cat || !a.logit || !a.prob || a.wide_off < 0)
    return (int)hipErrorInvalidValue;
  if (a.label && (!a.loss || !a.hit || !a.sums)) return (int)hipErrorInvalidValue;
  // 4-byte loads of the bf16 shadow's pairs, 8-byte loads of the ids, 8-byte accumulators
  if ((p[1] & 3) || (a.woff[1] & 1) || (a.woff[2] & 1) || (a.woff[3] & 1) || (p[0] & 3) || (p[2] & 3) || (p[3] & 7) ||
      (p[9] & 7))
    return (int)hipErrorInvalidValue;
  const long nacc = (1L + a.slice_card) * 3;
  a.hist = (unsigned*)(a.sums + nacc);
  int dev = 0, cus = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess || cus < 1) return (int)(e != hipSuccess ? e : hipErrorInvalidDevice);
  const long trips = (a.ntiles + 3) / 4;
  long grid = iv[14] > 0 ? iv[14] : 2L * cus;
  if (grid > trips) grid = trips;
  static bool attr[64] = {};  // per device: the kernel's dynamic LDS exceeds the 64 KB default limit
  if (dev < 0 || dev >= 64 || !attr[dev]) {
    e = hipFuncSetAttribute((const void*)taxi_eval_k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    if (e != hipSuccess) return (int)e;
    if (dev >= 0 && dev < 64) attr[dev] = true;
  }
  if (a.label) {
    const long n64 = nacc + (1L + a.slice_card) * NB;  // (2 NB uint32 = NB uint64 per slice)
    long cg = (n64 + 255) / 256;
    if (cg > 1024) cg = 1024;
    hipLaunchKernelGGL(taxi_eval_clear_k, dim3((unsigned)cg), dim3(256), 0, st, a.sums, n64);
  }
  hipLaunchKernelGGL(taxi_eval_k, dim3((unsigned)grid), dim3(NT), LDS_BYTES, st, a);
  return (int)hipGetLastError();
}

extern "C" int hopsx_taxi_eval_bins() { return taxiev::NB; }
