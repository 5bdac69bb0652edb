// hopsx: the flagship MNIST CNN training step as ONE persistent launch per `nsteps` steps (gfx950).
//
// Model (reference E3/E5, notebooks/ml/Distributed_Training/mirrored_strategy/
// mirroredstrategy_mnist_example.ipynb:189-207): uint8 28x28 -> x/255 - .5 -> Conv32 k2 relu ->
// Conv64 k2 relu -> MaxPool2 -> Dropout(.01) -> Dense128 relu -> Dense10 -> sparse softmax CE
// (mean over the batch) -> Adadelta(lr, rho, eps) (:210-222 compile/fit).  B = 32 images per step.
//
// Why one launch.  The whole step is ~1.35 GFLOP (0.5 us of MFMA time at bf16 peak) spread over six
// dependent ops: as separate kernels it is latency-bound (six launches, each re-reading its operands
// and the 1.38 M-parameter fc1 weight / Adadelta state from HBM: ~36 MB per step).  Here every
// workgroup keeps its share of the model ON CHIP for all `nsteps` steps and hands off only the small
// activations between phases.
//
// Partition (the design decision everything else follows from): workgroup p < 169 owns pooled
// position p = (ph, pw) of the 13x13 map, for all 32 images and all 64 channels.  Then
//   * its conv1 -> conv2 -> pool receptive field is a private 4x4 input patch (conv1 and conv2 are
//     recomputed per position, no halo exchange);
//   * the fc1 weight columns it multiplies (W1[:, p*64 .. p*64+63], 8192 params) are touched by no
//     other workgroup: forward partial product, weight gradient AND the Adadelta update are local,
//     and its fp32 master + two Adadelta accumulators live in the lane registers of the fc1 wgrad
//     MFMA output layout (96 VGPRs per lane) for the whole launch (written back once at the end);
//   * the fc1 input gradient for its 64 pooled inputs is local too, so the whole conv backward is.
// What must cross workgroups per step (4 hand-offs, the critical path):
//   A  fc1 partial sums  [32 x 128] fp32 per position  -> 32 head workgroups (one per image) reduce
//      them in a fixed order, add the bias, relu, Dense10, softmax CE, dlogits, dh;
//   B  dh (+ h, dlogits, loss) of each image -> every position workgroup (and every head: each head
//      recomputes the fc2 / fc1-bias gradient from all 32 payloads and applies the SAME Adadelta
//      update to its replicated copy of those 1,418 params — bit-identical, no reduction hop);
//   C  conv-parameter gradient partials (8,416 fp32) per position -> 132 slice owners (64 params = two
//      128-byte lines each) reduce over the 169 partials in a fixed order and run Adadelta on their slice;
//   D  the updated conv parameters -> every position workgroup (next step's forward).
// Hand-off form: MI355X_MICROARCH.md "Valid forms" table, row 1 (cdna_hip_programming §6 G16 R1):
// payload stored write-through (16-B `sc1` buffer stores), every storing wave drains vmcnt, a
// workgroup barrier, ONE lane stores the flag (agent-scope relaxed = `global_store sc1`); the consumer
// polls the flags relaxed from one wave, then a barrier, then EVERY payload load is an `sc1` buffer
// load.  Flag epochs grow across launches (epoch = base + step + 1, the 64-bit base kept after the flag
// rows and advanced by nsteps at the end of each launch), so no memset precedes a launch.  Every
// poll is bounded (wall clock) and also watches a sticky error word, so a fault drains the grid.
// Payload buffers are double-buffered by step parity.
// The fan-in C (169 partials -> each slice owner) is consumed progressively (gather_rows below,
// HOPSX_PERSIST_PROG): each wave polls the flags of the producers whose rows its own lanes load and issues a
// row's sc1 loads as soon as its own poll has shown that row's flag, whatever the order of arrival, so only the
// last producers' rows are loaded after the last flag; the barrier moves behind the (unchanged, fixed-order)
// sum.  Producers, payload, flags and epochs are those of the flag form.  (The same for the heads' fan-in A
// measured SLOWER, 24.2 vs 23.6 us/step: the heads spin on A for ~10 us, and a poll issued behind a batch of
// row loads returns only after them, so the last flag is seen later than by the bare poll;
// profiles/r9_persist_progressive.txt.)
// B towards the positions is the exception (the slowest hop in the flag form: 201 workgroups on one flag
// line, a drain in the producer, a second round trip in the consumer): each head also stores dh as 64
// 8-byte {bf16 pair, epoch} granules that are their own flag (G16 R2, "tagged granules" below), and the
// positions wait on those tags; the fp32 payload + FL_B flag stay for the heads' own fc2 update.
//
// Determinism: no float atomics anywhere — every cross-workgroup sum is a fixed-order loop, so two
// runs from the same state are bit-identical.
#include "common.h"
#include "mnist_cnn.h"
#include "optim_core.h"
#include "wg_prims.h"

namespace mnistp {
using namespace wgp;
using namespace mnist_cnn;  // layer sizes, PH / NPOS / KIN, the W1S / W2S / C1S / PLS row strides

constexpr int B = 32;  // images per step
// (one position workgroup per pooled position: NPOS of them)
constexpr int NCONV = C2 * 128 + C2 + C1 * 4 + C1;  // 8416 conv params: [w2 | b2 | w1 | b1]
constexpr int OFF_B2 = C2 * 128, OFF_W1 = OFF_B2 + C2, OFF_B1 = OFF_W1 + C1 * 4;
// A slice is two whole 128-byte lines of a slabC row (the rows are 128-byte aligned: NCONV * 4 = 263 * 128), so
// an owner fetches exactly the lines it uses and no line is fetched by two owners; the conv2 weights end on a
// slice boundary (OFF_B2 = 128 slices), so an owner publishes either one whole bf16 line of D or two whole fp32
// lines.  Which workgroup owns an element changes no bit: its sum over the positions and its Adadelta are
// element-wise
constexpr int SLICE = 64, NSLICE = (NCONV + SLICE - 1) / SLICE;  // 132 slice owners (131 is half filled)
constexpr int NRED = 19;                                           // partial groups in the slice reduce
constexpr int NKC = (NPOS + NRED - 1) / NRED;                      // 9 partials per group: pp = g + NRED k
constexpr int NQ = SLICE / 4;                                      // 16-byte quads per slice row
constexpr int NHEAD = B;
constexpr int GRID = NPOS + NHEAD;  // 201 workgroups, one per CU
constexpr int PAY = 272;            // head payload floats
constexpr int PAY_DH = 0, PAY_H = 128, PAY_DL = 256, PAY_LOSS = 268, PAY_COR = 269;
constexpr int FL_A = 0, FL_B = 256, FL_C = 512, FL_D = 768, FL_WORDS = 1024;
constexpr int FL_EPOCH = FL_WORDS - 2;  // 64-bit epoch base after the flag rows (8-B aligned)
// D payload (updated conv parameters): the conv2 weights as bf16 (what the MFMAs read), then the 224
// small fp32 parameters [b2 | conv1 w | conv1 b]
constexpr int D_F32 = OFF_B2 * 2;                 // byte offset of the fp32 part
constexpr int D_BYTES = D_F32 + (NCONV - OFF_B2) * 4;
// Tagged hand-off B (dh for the positions): 8-byte granules {value, tag = the step's epoch} that are their own
// flag (cdna_hip_programming §6 G16 R2), each written by ONE 8-byte write-through store and read by 8-byte
// sc1 loads, double-buffered by step parity: [2][32 images][64] {bf16 dh[2l] | bf16 dh[2l+1] << 16, tag}.
// They live behind the flag rows in the flag allocation (zeroed with it: a tag of 0 is never an epoch).
// (The same form for D, the conv parameters, measured SLOWER than its flag form — 26.4 vs 25.6 us/step: D's
// hop is hidden behind the fc1 Adadelta, and 34 KB of 8-byte loads per reader cost more than the poll + 17 KB
// of 16-byte loads they replace; profiles/r7_persist_tagged.txt.)
constexpr int TGB_N = NHEAD * (HID / 2);  // 2048 granules (16 KB) per parity
constexpr int TG_WORDS = 2 * 2 * TGB_N;   // 32-bit words of the tag region
static_assert(FL_WORDS % 2 == 0 && TGB_N % 256 == 0, "granules are 8-B aligned; every thread owns TGB_N / 256");
// Waits filled with work that is ready early and needs nothing from the hand-off waited for (HOPSX_PERSIST_FILL, one
// bit per part, in Args::hand).  No float operation changes its operands or its order: only where it runs
constexpr int HAND_FILL_C = 1 << 16;     // owners of <false>: the fc1 slice Adadelta, a chunk per poll of the C gather
constexpr int HAND_FILL_KEEP = 1 << 17;  // the next step's dropout keep mask drawn in the B wait
constexpr int HAND_FMAX_SHIFT = 20;      // 4 bits: chunks that may run inside the C wait (HOPSX_PERSIST_FILL_MAX)
// The heads' A-to-B chain (head_wg; profiles/r18_persist_head_chain.txt).  Like the fills, nothing here changes a
// float operation's operands or order, and no producer, payload, flag, epoch or granule
constexpr int HAND_GATEA_SHIFT = 18;     // 2 bits: the one-line gate in front of the heads' A wait (HOPSX_PERSIST_GATE_A)
constexpr int HAND_HEAD_REGS = 1 << 24;  // the one-wave head's operands in registers from the top of the step
constexpr int HAND_HEAD_TREE = 1 << 25;  // its ten logits by wave_sum_tree (HOPSX_PERSIST_HEAD_CHAIN bits 1, 2)
// The positions' local compute staged wave-locally (position_wg; profiles/r21_persist_wave_local.txt,
// HOPSX_PERSIST_WLOCAL, one bit per part).  Where the thread-to-data maps make the wave that writes an LDS tile the
// only wave that reads it, the workgroup barrier between the two is a wave-level ordering point (wave_lds_order), and
// a wave publishes its own block of A and of C's part 1 without waiting for the others.  No float operation, payload
// byte, flag or epoch changes; 0 is the parent's path
constexpr int HAND_WL_FWD = 1 << 4;  // XIN fill -> conv1 -> conv2 without workgroup barriers
constexpr int HAND_WL_A = 1 << 5;    // a wave publishes its own 32 x 32 block of A
constexpr int HAND_WL_BWD = 1 << 6;  // pool backward -> conv2 wgrad -> C part 1 per wave, ONE barrier before the conv2 dgrad
// -DHOPSX_PERSIST_WLOCAL_FIXED=n (tools/persist_isa.py only): the parts are n at compile time, so the assembly has
// one arm of every branch on them and the static instruction table is that of ONE path
#ifdef HOPSX_PERSIST_WLOCAL_FIXED
#define HOPSX_WL_HAND(a) (((HOPSX_PERSIST_WLOCAL_FIXED) & 7) << 4)
#else
#define HOPSX_WL_HAND(a) ((a).hand)
#endif
constexpr int NLINE_A = (NPOS + 31) / 32;  // 128-byte lines of the A flag row
// the 32 lane-owned fc1 updates of a step in chunks of FCH, in the order of the whole update (ii, j, r).  A chunk has
// to stay well below a flag round trip (it runs between a poll's loads and the ballot that consumes them): 4 updates
// are ~60 VALU, 8 of them quarter-rate (sqrt, rsq)
constexpr int FCH = 4, NFCH = 32 / FCH;
static_assert(32 % FCH == 0 && NFCH <= 15, "whole chunks; the cap fits its 4 bits of Args::hand");

// LDS row strides (bf16 elements) of the backward-only images, by mnist_cnn.h's rule
constexpr int DHS = row_stride(HID), DCS = row_stride(4 * B);
static_assert(DHS == 136 && DCS == 136, "strides the kernel was tuned with");

// position-workgroup LDS map (bytes, every offset a multiple of 16)
constexpr int L_W1 = 0;                           // bf16 [128 n][W1S]   fc1 slice
constexpr int L_W2 = L_W1 + HID * W1S * 2;        // bf16 [64 co][W2S]  conv2 weights (OHWI rows)
constexpr int L_CW1 = L_W2 + C2 * W2S * 2;        // f32  [32][4]       conv1 weights
constexpr int L_CB1 = L_CW1 + C1 * 4 * 4;         // f32  [32]
constexpr int L_CB2 = L_CB1 + C1 * 4;             // f32  [64]
constexpr int L_XIN = L_CB2 + C2 * 4;             // f32  [32 b][16]    input patch
constexpr int L_C1 = L_XIN + B * 16 * 4;          // bf16 [32 b][9 pos][C1S] conv1 output
constexpr int L_POOL = L_C1 + B * 9 * C1S * 2;    // bf16 [32 b][PLS]   pooled (+dropout)
constexpr int L_AM = L_POOL + B * PLS * 2;        // u8   [32 b][64]    argmax tap / 0xFF = no grad
constexpr int L_DH = L_AM + B * C2;               // bf16 [32 b][DHS]
constexpr int L_DC2 = L_DH + B * DHS * 2;         // bf16 [64 co][DCS] conv2 output grad, (b,q) cols
constexpr int L_STG = L_DC2 + C2 * DCS * 2;       // f32  staging: A partial [32][128] / C grads [8416]
constexpr int L_RED = L_STG + NCONV * 4;          // f32  [NRED][SLICE] slice reduce / conv1 grad halves
constexpr int L_SL = L_RED + NRED * SLICE * 4;    // f32  [3][SLICE] owned conv slice: master, s1, s2
constexpr int L_KEEP = L_SL + 3 * 64 * 4;         // u8   [32 b][64] next step's dropout keep mask
constexpr int LDS_BYTES = L_KEEP + B * C2;

// head-workgroup LDS map (aliases the same allocation)
constexpr int H_W2 = 0;                       // f32 [3][10*128] fc2 weight: master, s1, s2
constexpr int H_B2 = H_W2 + 3 * NCLS * HID * 4;  // f32 [3][16]
constexpr int H_B1 = H_B2 + 3 * 16 * 4;       // f32 [3][128]
constexpr int H_RED = H_B1 + 3 * HID * 4;     // f32 [8][128]
constexpr int H_H = H_RED + 8 * HID * 4;      // f32 [128]
constexpr int H_LOG = H_H + HID * 4;          // f32 [16]
constexpr int H_PAY = H_LOG + 16 * 4;         // f32 [PAY]
constexpr int H_ALL = H_PAY + PAY * 4;        // f32 [32][PAY]
constexpr int H_END = H_ALL + NHEAD * PAY * 4;
constexpr int H_DHS = H_END;                  // bf16 [32][DHS] dh staging (head 0, data-parallel)
static_assert(H_DHS + B * DHS * 2 <= LDS_BYTES, "head LDS map must fit the position map");

// ---- data-parallel exchange (DP instantiation, world > 1) ----
// Each rank owns one uncached (UC) exchange buffer and one UC flag page, IPC-mapped by every peer.
// A producer PUSHES its payload into every peer's buffer at slot [its rank] (system-scope write-through
// stores), drains, and raises its flag word in every peer's page; a consumer polls its OWN page and
// reads its OWN buffer (local memory, no L2 copies to go stale).  Flags carry a global step epoch that
// grows across launches (never reset), payloads are double-buffered by step parity.
constexpr int XMAX = 8;                                         // ranks (one node)
constexpr long XS_POOL = (long)NPOS * 4 * 64 * 16;              // fc1-wgrad B fragments of all positions
constexpr long XS_DHT = 8L * 64 * 16;                           // fc1-wgrad A fragments (dh^T), 8 n-blocks
constexpr int NFC2 = NCLS * HID + HID + NCLS, NFC2P = 1424;     // [fc2 w | fc1 b | fc2 b] gradient
constexpr long XS_FC2 = NFC2P * 4;
constexpr long XS_CONV = (long)NSLICE * SLICE * 4;              // conv slice gradient sums
constexpr long XO_POOL = 0, XO_DHT = XO_POOL + 2L * XMAX * XS_POOL, XO_FC2 = XO_DHT + 2L * XMAX * XS_DHT,
               XO_CONV = XO_FC2 + 2L * XMAX * XS_FC2, X_BYTES = XO_CONV + 2L * XMAX * XS_CONV;
constexpr int XF_POOL = 0, XF_H = XMAX * NPOS, XF_CONV = XF_H + XMAX, XF_WORDS = XF_CONV + XMAX * NSLICE;
static_assert(NFC2 <= NFC2P && NFC2P % 4 == 0 && X_BYTES < 0x7fffffffL, "exchange geometry");
static_assert(LDS_BYTES <= 160 * 1024, "one workgroup per CU: 160 KiB LDS");
static_assert(L_RED + NRED * SLICE * 4 <= L_SL && 2 * 32 * 5 * 4 <= NRED * SLICE * 4, "reduce scratch");
static_assert(SLICE * 4 % 128 == 0 && NCONV * 4 % 128 == 0, "a slice row is whole 128-byte lines of an aligned slabC row");
static_assert(OFF_B2 % SLICE == 0 && D_F32 % 128 == 0 && D_BYTES % 128 == 0, "no slice straddles the bf16 / fp32 parts of D");
static_assert(NSLICE * SLICE >= NCONV && NSLICE <= NPOS && SLICE == 64, "slice geometry: one wave updates a slice");
// the owners' gather: wave w (of 4) loads groups 4w .. 4w + 3, 16 lanes (one quad each) per group, so one wave
// instruction reads 4 whole rows; groups 16 .. NRED - 1 are a second item on the last 16 lanes of waves
// 0 .. NRED - 17
static_assert(NQ == 16 && NRED > 16 && NRED - 16 <= 3 && 5 * NKC <= 64 && 2 * NKC <= 32 && NRED * (NKC - 1) < NPOS,
              "gather geometry: at most 5 groups' flags per wave, one per lane; both items' rows in one pend mask");

struct Args {
  float* master;      // arena fp32 parameters
  bf16_raw* shadow;   // arena bf16 copy the other kernels read
  float* s1;          // Adadelta E[g^2]
  float* s2;          // Adadelta E[dx^2]
  long off[8];        // arena offsets: conv1.w conv1.b conv2.w conv2.b fc1.w fc1.b fc2.w fc2.b
  const unsigned char* xs;  // uint8 [nbatch][32][28][28]
  const long long* ys;      // int64 [nbatch][32]
  long nbatch;
  long long* cursor;         // next batch index (advanced by nsteps at the end)
  unsigned long long* rng;   // {seed, step counter} (dropout key; advanced by nsteps)
  float* step_dev;           // optimizer step count (advanced by nsteps), may be null
  const float* hp_dev;       // device hyper-parameters (OptHP layout), may be null
  float* slabA;  // [2][169][32][128]
  float* slabB;  // [2][32][PAY]
  float* slabC;  // [2][169][NCONV]
  float* slabD;  // [2][D_BYTES / 4]
  unsigned* flags;  // [FL_WORDS + TG_WORDS]: flag rows + the epoch base, then the tag granules (zeroed once
                    // at allocation)
  unsigned* err;    // sticky error word (0 = ok)
  float* out;       // [nsteps][2]: mean loss, correct count
  unsigned long long* dbg;  // optional [GRID][nsteps][16] wall-clock phase stamps
  OptHP hp;
  float drop_p, xscale, xshift;
  unsigned salt;
  int nsteps;
  int acquire;  // 1: agent-scope acquire after every poll (diagnostic; the sc1 form needs none)
  long long tmo;  // wall-clock ticks a poll waits before it declares the producer lost
  long long tmo0;  // the same for step 0's purely local waits (co-residency: HOPSX_PERSIST_START_MS)
  int pollw, stagger;  // waves polling a hand-off wait and their start offsets (HOPSX_PERSIST_POLLW / _STAGGER)
  int pollw_a, pollw_b, pollw_c, pollw_d;  // per hand-off (HOPSX_PERSIST_POLLW_A.._D, default POLLW; C: 4)
  int head1w;          // 1: one wave computes the head from registers and publishes B (HOPSX_PERSIST_HEAD1W)
  // hand-off form, one word (one scalar register for the whole launch): bit 0: the positions read dh (B) from
  // tagged granules, not the flag form (HOPSX_PERSIST_TAGGED); bit 1: a flag poll loads the error word with
  // its flags, one round trip (HOPSX_PERSIST_POLL1); bit 3: the slice owners load a partial of C as soon as its
  // flag is there (HOPSX_PERSIST_PROG bit 1); bits 8..15: heads whose tag opens the B wait's gate
  // (HOPSX_PERSIST_GATE); bits 16..17: the waits that are filled with work that is ready early
  // (HOPSX_PERSIST_FILL, HAND_FILL_*); bits 20..23: chunks of the fc1 update the owners may run inside the C wait
  // (HOPSX_PERSIST_FILL_MAX); bits 18..19: the gate in front of the heads' A wait (HOPSX_PERSIST_GATE_A); bits 24..25:
  // the one-wave head's operands in registers, its logits by wave_sum_tree (HOPSX_PERSIST_HEAD_CHAIN, HAND_HEAD_*);
  // bits 4..6: the positions' wave-local staging (HOPSX_PERSIST_WLOCAL, HAND_WL_*)
  int hand;
  int gate_a_tk;  // wall-clock ticks the A gate watches its line before it gives way to the full wait (_GATE_A_US)
  float inv_gb;   // 1 / global batch (world * B): the loss is the mean over every replica's images
  // data parallel (DP instantiation)
  int world, rank;
  int loopback;                 // 1: one process plays every rank (peers = this rank's own buffers)
  int xfence;                   // 1: system-scope release fence before raising peer flags
  long long* xstep;             // global step counter (epoch base of the exchange flags)
  unsigned char* xbuf[XMAX];    // exchange buffers of ranks 0..world-1 (own at [rank])
  unsigned* xflag[XMAX];        // flag pages of ranks 0..world-1
};

// Payload path of the hand-offs: write-through 16-B / 8-B stores and L1-bypassing 16-B loads (bst16<SC1>,
// bst8<SC1>, bld16<SC1>); cross-rank exchange path: the same family at system scope (<SYS>); flag words:
// flag_store / flag_load (agent scope), xflag_store / xflag_load (system scope).  All in wg_prims.h.

// slot a push lands in: the producer's rank (loopback: the simulated peer's, so every slot fills)
__device__ __forceinline__ int xslot(const Args& a, int peer) { return a.loopback ? peer : a.rank; }

// Wave 0 polls flags[0..n) until every word equals `epoch` (relaxed sc1 loads + s_sleep); gives up
// on the sticky error word or after a.tmo ticks (recording `code`).  Returns the verdict to the
// whole workgroup (uniform).
// pollw > 1 (HOPSX_PERSIST_POLLW): that many waves poll, their first polls staggered by `stagger` x 64
// cycles, so a flag that lands between two polls of one wave is seen by the next wave's poll — the
// detection delay shrinks from ~half a poll round trip toward ~half of that over pollw.  The first
// wave to see every flag (or the error) tells the others through the LDS word s_ok[1], set to this
// wait's `code` (unique per phase and step, never 0); s_ok[0] carries the verdict as before.
// poll1 (HOPSX_PERSIST_POLL1): the error word is loaded WITH the flags of the same iteration (one wait for
// both), so a poll iteration is one memory round trip instead of two dependent ones; the flags are still
// judged first, so a hand-off that has arrived wins over an error raised meanwhile, as before.
__device__ __forceinline__ bool wait_all(const unsigned* flags, int n, unsigned epoch, unsigned* err, unsigned code,
                                      int acquire, int* s_ok, long long tmo, int pollw = 1, int stagger = 0,
                                      int poll1 = 0) {
  if (pollw <= 1) {
    if (threadIdx.x < 64) {
      const int lane = threadIdx.x;
      int good = 1;
      const long long t0 = wall_clock64();
      for (unsigned spins = 0;; ++spins) {
        int ok = 1;
        unsigned e = poll1 ? flag_load(err) : 0u;
        for (int k = lane; k < n; k += 64) ok &= flag_load(flags + k) == epoch;
        if (__all(ok)) break;
        if (!poll1) e = flag_load(err);
        if (__builtin_amdgcn_readfirstlane(e) != 0u) {
          good = 0;
          break;
        }
        if ((spins & 15u) == 15u && wall_clock64() - t0 > tmo) {
          if (lane == 0) atomicCAS(err, 0u, code);
          good = 0;
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
      if (acquire && good) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      drain();
      if (lane == 0) *s_ok = good;
    }
    __syncthreads();
    const int g = *s_ok;
    return g != 0;
  }
  volatile int* gen = s_ok + 1;
  const int wave = threadIdx.x >> 6;
  if (wave < pollw) {
    const int lane = threadIdx.x & 63;
    int good = 1;
    // (the stagger checks the done word too: when the flags are already there, wave 0's first poll ends
    // the wait and the later waves must not sleep out their offsets before the barrier)
    for (int d = 0; d < wave * stagger && __builtin_amdgcn_readfirstlane(*gen) != (int)code; ++d)
      __builtin_amdgcn_s_sleep(1);
    const long long t0 = wall_clock64();
    for (unsigned spins = 0;; ++spins) {
      if (__builtin_amdgcn_readfirstlane(*gen) == (int)code) break;  // another wave saw it
      int ok = 1;
      unsigned e = poll1 ? flag_load(err) : 0u;
      for (int k = lane; k < n; k += 64) ok &= flag_load(flags + k) == epoch;
      if (__all(ok)) {
        if (lane == 0) {
          s_ok[0] = 1;
          *gen = (int)code;
        }
        break;
      }
      if (!poll1) e = flag_load(err);
      if (__builtin_amdgcn_readfirstlane(e) != 0u) good = 0;
      if ((spins & 15u) == 15u && wall_clock64() - t0 > tmo) {
        if (lane == 0) atomicCAS(err, 0u, code);
        good = 0;
      }
      if (!good) {
        if (lane == 0) {
          s_ok[0] = 0;
          *gen = (int)code;
        }
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    if (acquire) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    drain();
  }
  __syncthreads();
  const int g = s_ok[0];
  return g != 0;
}

// Wave 0 polls this rank's flag page until word base + r * stride has reached `epoch` for every peer
// r != rank (the epoch grows across launches: "reached" is a wrap-safe >=).  Same failure handling
// and uniform verdict as wait_all.
__device__ __forceinline__ bool wait_peers(const Args& a, int base, int stride, unsigned epoch, unsigned code,
                                        int* s_ok) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const unsigned* page = a.xflag[a.rank];
    int good = 1;
    const long long t0 = wall_clock64();
    for (unsigned spins = 0;; ++spins) {
      const bool mine = lane < a.world && lane != a.rank;
      unsigned e = (a.hand & 2) ? flag_load(a.err) : 0u;
      const int ok = !mine || (int)(xflag_load(page + base + lane * stride) - epoch) >= 0;
      if (__all(ok)) break;
      if (!(a.hand & 2)) e = flag_load(a.err);
      if (__builtin_amdgcn_readfirstlane(e) != 0u) {
        good = 0;
        break;
      }
      if ((spins & 15u) == 15u && wall_clock64() - t0 > a.tmo) {
        if (lane == 0) atomicCAS(a.err, 0u, code);
        good = 0;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    drain();
    if (lane == 0) *s_ok = good;
  }
  __syncthreads();
  const int g = *s_ok;
  return g != 0;
}
// raise this rank's flag word base + slot * stride in every peer's page (after the payload drained)
// The payload stores are system-scope write-through (sc0 sc1) and drained (vmcnt 0) by every storing
// wave before this: that completes them at the system coherence point, the release for exactly these
// stores.  The optional fence (HOPSX_PERSIST_XFENCE=1) also writes back other dirty L2 lines.
__device__ __forceinline__ void raise_peers(const Args& a, int base, int stride, unsigned epoch) {
  if (a.xfence) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope: buffer_wbl2 sc0 sc1 + drain
  const int r = threadIdx.x & 63;
  if (r < a.world && r != a.rank) xflag_store(a.xflag[r] + base + xslot(a, r) * stride, epoch);
}

// Adadelta (optim_core.h upd<3>, rho = a, eps = b) with the hardware square root / reciprocal square
// root (1 ulp) instead of the correctly rounded sqrt + division sequences: ~8 instead of ~35 VALU ops
// an element, and the fc1 slice update (32 elements a lane) sits on the step's critical path
__device__ __forceinline__ float adadelta(float w, float g, float& s1, float& s2, const OptHP& h) {
  g = fmaf(h.wd, w, g);
  s1 = fmaf(h.a, s1, (1.f - h.a) * g * g);
  const float delta = g * __builtin_amdgcn_sqrtf(s2 + h.b) * __builtin_amdgcn_rsqf(s1 + h.b);
  s2 = fmaf(h.a, s2, (1.f - h.a) * delta * delta);
  return fmaf(-h.lr, delta, w);
}

__device__ __forceinline__ unsigned ecode(int phase, int s) {
  return 0x80000000u | ((unsigned)phase << 24) | (((unsigned)s & 0xFFFu) << 12) | (blockIdx.x & 0xFFFu);
}

__device__ __forceinline__ long conv_idx(const Args& a, int j) {
  if (j < OFF_B2) return a.off[2] + j;
  if (j < OFF_W1) return a.off[3] + (j - OFF_B2);
  if (j < OFF_B1) return a.off[0] + (j - OFF_W1);
  return a.off[1] + (j - OFF_B1);
}

// Ordering point between LDS stores and LDS reads of ONE wave (other lanes' data, nothing another wave wrote): the
// compiler moves no LDS access across it (it sees per-thread addresses that do not alias and would otherwise hoist the
// reads), and the wave waits until its own LDS operations have completed
__device__ __forceinline__ void wave_lds_order() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
// `wl` (workgroup-uniform: a bit of Args::hand) chooses the wave-level point over the workgroup barrier it stands for
__device__ __forceinline__ void wave_or_wg(bool wl) {
  if (wl) wave_lds_order();
  else __syncthreads();
}

__device__ __forceinline__ void stamp(const Args& a, int s, int ph) {
  if (a.dbg && threadIdx.x == 0) a.dbg[((long)blockIdx.x * a.nsteps + s) * 16 + ph] = (unsigned long long)wall_clock64();
}

// ---- tagged granules (hand-off B, heads -> positions): the data is the flag ----
// ONE aligned 8-byte write-through (sc1) store per granule and lane: value in the low word, tag in the high
__device__ __forceinline__ void granule_store(unsigned long long* g, unsigned epoch, unsigned value) {
  __hip_atomic_store((gu64*)g, ((unsigned long long)epoch << 32) | value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long granule_load(const unsigned long long* g) {
  return __hip_atomic_load((gu64*)g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // global_load_dwordx2 sc1
}
// The cheap first stage of the B wait (the positions wait ~7 us there: 169 workgroups sweeping 16 KB each
// all that time would load the fabric).  Wave 0 polls ONE granule per head — lane l < 32 image l's granule
// `gi`, 32 different lines — with s_sleep, until `need` of them carry the epoch; same error word, wall-clock
// bound and uniform verdict as wait_all.  It only opens the sweep: the sweep checks every granule's tag.
__device__ __forceinline__ bool gate_tags(const unsigned long long* g, int gi, unsigned epoch, int need, unsigned* err,
                                       unsigned code, int* s_ok, long long tmo) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const bool mine = lane < NHEAD;
    int good = 1;
    const long long t0 = wall_clock64();
    for (unsigned spins = 0;; ++spins) {
      const unsigned e = flag_load(err);
      const unsigned long long x = mine ? granule_load(g + lane * (HID / 2) + gi) : 0ull;
      const bool hit = mine && (unsigned)(x >> 32) == epoch;
      if (__popcll(__ballot(hit)) >= need) break;
      if (__builtin_amdgcn_readfirstlane(e) != 0u) {
        good = 0;
        break;
      }
      if ((spins & 15u) == 15u && wall_clock64() - t0 > tmo) {
        if (lane == 0) atomicCAS(err, 0u, code);
        good = 0;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    if (lane == 0) *s_ok = good;
  }
  __syncthreads();
  const int v = *s_ok;
  return v != 0;
}
// Every thread owns granules tid + 256 k (k < N) of g[0 .. 256 N): it loads them (all in flight, 8-byte sc1
// loads to registers), hands the value of each whose tag is the epoch to put(index, value) and re-reads only
// the others, until the whole workgroup has all of them; one barrier at the end (put writes LDS).  The error
// word travels with each pass's loads (one round trip per pass); failure handling as wait_all, the verdict
// through the LDS word s_fail (0 until a wave gives up), uniform.
template <int N, class F>
__device__ __forceinline__ bool sweep_tags(const unsigned long long* g, int tid, unsigned epoch, unsigned* err,
                                        unsigned code, int* s_fail, long long tmo, F put) {
  unsigned pend = (1u << N) - 1u;
  unsigned long long x[N];
#pragma unroll
  for (int k = 0; k < N; ++k) x[k] = granule_load(g + tid + 256 * k);  // the first pass: every granule
  unsigned e = flag_load(err);
  const long long t0 = wall_clock64();
  for (unsigned spins = 0;; ++spins) {
#pragma unroll
    for (int k = 0; k < N; ++k)
      if (((pend >> k) & 1u) && (unsigned)(x[k] >> 32) == epoch) {
        put(tid + 256 * k, (unsigned)x[k]);
        pend &= ~(1u << k);
      }
    if (!__any(pend != 0u)) break;
    bool bad = __builtin_amdgcn_readfirstlane(e) != 0u;
    if (!bad && (spins & 15u) == 15u && wall_clock64() - t0 > tmo) {
      if ((threadIdx.x & 63) == 0) atomicCAS(err, 0u, code);
      bad = true;
    }
    if (bad) {
      if ((threadIdx.x & 63) == 0) *s_fail = 1;
      break;
    }
#pragma unroll
    for (int k = 0; k < N; ++k)
      if ((pend >> k) & 1u) x[k] = granule_load(g + tid + 256 * k);
    e = flag_load(err);
  }
  __syncthreads();
  const int f = *s_fail;
  return f == 0;
}

// ---- progressive fan-in (hand-off C): a row is loaded as soon as ITS flag is there ----
// The flag form reads a fan-in payload only after the LAST producer's flag (poll, barrier, then every load), although
// the producers finish up to a microsecond apart and almost every row has long been in memory by then.  Here every
// wave polls the flags of exactly the producers whose rows its own lanes load — one flag per lane (`flag`, `mine`),
// the error word in the same round trip — and the ballot of "flag == epoch" is the arrived set; bit `shift` + k of
// it is this thread's row k.  Each thread then issues load(k) for every row of its `pend` mask that has arrived,
// in any order of arrival (no in-order prefix: one late producer holds back only its own row), k static (the
// pend-mask idiom of sweep_tags: the rows stay in registers), and polls again, with s_sleep, until no lane of the
// wave has a row pending.  After the last flag only that flag's rows are still to load: one round trip.
// Still row 1 of the "Valid forms" table: every load of handed-off bytes is an sc1 load issued by a wave after its
// OWN poll has shown that producer's flag; no wave relies on another's poll.  Failure handling as sweep_tags: every
// poll is bounded by `tmo` (recording `code`) and watches the sticky error word; a wave that gives up sets *s_fail.
// No barrier in here: the caller reads *s_fail (uniform) behind the barrier that follows its reduce.
// fill(): work of the caller's that is ready and needs nothing from the hand-off, run between issuing a poll's two
// loads and the ballot that consumes them, i.e. inside the round trip the wave would otherwise sit out; it returns
// whether it did anything (wave-uniform), and a poll whose fill did takes no s_sleep.  It must stay shorter than a
// flag round trip (or the last flag is seen late) and must not touch what load() writes.
template <int NK, class L, class F>
__device__ __forceinline__ void gather_rows(const unsigned* flag, bool mine, int shift, unsigned pend, unsigned epoch,
                                            unsigned* err, unsigned code, int* s_fail, long long tmo, L load, F fill) {
  const long long t0 = wall_clock64();
  for (unsigned spins = 0;; ++spins) {
    const unsigned e = flag_load(err);
    const unsigned f = mine ? flag_load(flag) : 0u;
    __builtin_amdgcn_sched_barrier(0);  // (the loads are issued ahead of the fill, their wait stays behind it)
    const bool filled = fill();
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long here = __ballot(mine && f == epoch);
    const unsigned now = pend & (unsigned)(here >> shift);
#pragma unroll
    for (int k = 0; k < NK; ++k)
      if ((now >> k) & 1u) load(k);
    pend &= ~now;
    if (!__any(pend != 0u)) break;
    bool bad = __builtin_amdgcn_readfirstlane(e) != 0u;
    if (!bad && (spins & 15u) == 15u && wall_clock64() - t0 > tmo) {
      if ((threadIdx.x & 63) == 0) atomicCAS(err, 0u, code);
      bad = true;
    }
    if (bad) {
      if ((threadIdx.x & 63) == 0) *s_fail = 1;
      break;
    }
    if (!filled) __builtin_amdgcn_s_sleep(1);
  }
}

// ------------------------------------------------------------------------------------------------
// position workgroup p: conv1 -> conv2 -> pool -> fc1 partial; backward of all of it; fc1 slice
// Adadelta; conv-parameter slice owner
// ------------------------------------------------------------------------------------------------
template <bool DP>
__device__ __forceinline__ void position_wg(const Args& a, unsigned char* smem, int* s_ok, const OptHP& hp,
                                            long long cur0, unsigned long long seed, unsigned long long ctr0,
                                            long long xs0, unsigned long long eb) {
  const int p = blockIdx.x, ph = p / PH, pw = p - ph * PH;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int tq = fr >> 2, tp = fr & 3;
  bf16_raw* W1 = (bf16_raw*)(smem + L_W1);
  bf16_raw* W2 = (bf16_raw*)(smem + L_W2);
  float* CW1 = (float*)(smem + L_CW1);
  float* CB1 = (float*)(smem + L_CB1);
  float* CB2 = (float*)(smem + L_CB2);
  float* XIN = (float*)(smem + L_XIN);
  bf16_raw* C1 = (bf16_raw*)(smem + L_C1);
  bf16_raw* POOL = (bf16_raw*)(smem + L_POOL);
  unsigned char* AM = smem + L_AM;
  bf16_raw* DH = (bf16_raw*)(smem + L_DH);
  bf16_raw* DC2 = (bf16_raw*)(smem + L_DC2);
  float* STG = (float*)(smem + L_STG);
  float* RED = (float*)(smem + L_RED);
  float* SLm = (float*)(smem + L_SL);
  float* SL1 = SLm + 64;
  float* SL2 = SLm + 128;

  // ---- fc1 slice: lane-owned (rows n = (2w+ii)*16 + fq*4 + r, column co = j*16 + fr) ----
  float wm[2][4][4], g1[2][4][4], g2[2][4][4];
#pragma unroll
  for (int ii = 0; ii < 2; ++ii)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = (2 * w + ii) * 16 + fq * 4 + r, co = j * 16 + fr;
        const long ai = a.off[4] + (long)n * KIN + p * C2 + co;
        wm[ii][j][r] = a.master[ai];
        g1[ii][j][r] = a.s1[ai];
        g2[ii][j][r] = a.s2[ai];
        W1[n * W1S + co] = f2bf_hw(wm[ii][j][r]);
      }
  // ---- conv parameters (every position needs all of them) ----
  auto put_conv = [&](int j, float v) {
    if (j < OFF_B2) W2[(j >> 7) * W2S + (j & 127)] = f2bf_hw(v);
    else if (j < OFF_W1) CB2[j - OFF_B2] = v;
    else if (j < OFF_B1) CW1[j - OFF_W1] = v;
    else CB1[j - OFF_B1] = v;
  };
  {
    // every load in flight before the LDS stores: a load -> store loop waited out one memory round trip per
    // iteration (33 of them: the launch prologue measured 16 us, tools/persist_check.py "launch:")
    constexpr int NJ = (NCONV + 255) / 256;
    float cv[NJ];
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
      const int j = tid + 256 * q;
      cv[q] = j < NCONV ? a.master[conv_idx(a, j)] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
      const int j = tid + 256 * q;
      if (j < NCONV) put_conv(j, cv[q]);
    }
  }
  const bool owner = p < NSLICE;
  if (owner && tid < SLICE) {
    const int e = p * SLICE + tid;
    if (e < NCONV) {
      const long ci = conv_idx(a, e);
      SLm[tid] = a.master[ci];
      SL1[tid] = a.s1[ci];
      SL2[tid] = a.s2[ci];
    }
  }
  // ---- input patch: thread -> (image xb, patch row xr, column pair xh) ----
  const int xb = tid >> 3, xr = (tid >> 1) & 3, xh = tid & 1;
  auto xload = [&](int s) -> unsigned {
    const long bt = (long)((cur0 + s) % a.nbatch);
    const unsigned char* q = a.xs + (bt * B + xb) * 784 + (2 * ph + xr) * 28 + 2 * pw + 2 * xh;
    return *(const unsigned short*)q;
  };
  unsigned xv = xload(0);
  const float P = a.drop_p, inv = P > 0.f ? 1.f / (1.f - P) : 1.f;
  unsigned char* KEEP = smem + L_KEEP;
  // the dropout keep mask of step s for this position (common.h drop_key / uniform01 on the NHWC
  // index of the pooled element): it depends only on the step and KEEP is read by the conv2 forward epilogue
  // alone, so it is drawn while the previous step waits for B, where the positions idle (HAND_FILL_KEEP; without
  // it behind the previous step's fc1 update, where the owners have no slack left)
  auto draw_keep = [&](int s) {
    const unsigned long long ctr = ctr0 + (unsigned long long)s;
    const uint64_t dkey = (uint64_t)seed ^ ((uint64_t)a.salt * 0xD1B54A32D192ED03ull) ^
                          ((uint64_t)ctr * 0x8CB92BA72F3D8DD7ull);
    for (int e = threadIdx.x; e < B * C2; e += 256) {
      const int b = e >> 6, co = e & 63;
      const long gb = (long)a.rank * B + b;  // global image index: every replica draws its own masks
      KEEP[e] = P > 0.f ? (unsigned char)(uniform01(dkey, (uint64_t)((gb * NPOS + p) * C2 + co)) >= P) : 1;
    }
  };
  draw_keep(0);
  __syncthreads();

  for (int s = 0; s < a.nsteps; ++s) {
    const unsigned ep = (unsigned)(eb + (unsigned long long)s + 1ull);
    const int par = s & 1;
    // lane indices re-derived from an opaque zero every step: otherwise the compiler hoists every
    // LDS address of the step body out of the loop and runs out of registers (spills to scratch)
    int oz;
    asm volatile("v_mov_b32 %0, 0" : "=v"(oz));
    const int tid = threadIdx.x + oz, lane = tid & 63, w = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const int tq = fr >> 2, tp = fr & 3, xb = tid >> 3, xr = (tid >> 1) & 3, xh = tid & 1;
    stamp(a, s, 0);
    XIN[xb * 16 + xr * 4 + 2 * xh] = (float)(xv & 0xFFu) * a.xscale + a.xshift;
    XIN[xb * 16 + xr * 4 + 2 * xh + 1] = (float)(xv >> 8) * a.xscale + a.xshift;
    // XIN fill -> conv1 is wave-local: xb = tid >> 3 writes images 8w .. 8w + 7, conv1's bg = tid >> 5 reads images
    // 8w .. 8w + 7.  XIN's cross-wave readers are the conv1 weight gradient (images 16 mh ..), behind the barrier in
    // front of the fc1 partial product below, and it ends before the barrier behind RED; CW1 / CB1 were written
    // behind the D load's barrier
    wave_or_wg(HOPSX_WL_HAND(a) & HAND_WL_FWD);
    // ---- conv1 (VALU): 32 images x 3x3 positions x 32 channels ----
    {
      const int ci = tid & 31, bg = tid >> 5;
      const float k0 = CW1[ci * 4 + 0], k1 = CW1[ci * 4 + 1], k2 = CW1[ci * 4 + 2], k3 = CW1[ci * 4 + 3];
      const float bias = CB1[ci];
      f32x4 xq[4][4];  // the 4x4 patches of this thread's 4 images, all in flight before the first use
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int c = 0; c < 4; ++c) xq[u][c] = *(const f32x4*)(XIN + (bg * 4 + u) * 16 + 4 * c);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int b = bg * 4 + u;
        const f32x4* xi = xq[u];
#pragma unroll
        for (int py = 0; py < 3; ++py)
#pragma unroll
          for (int px = 0; px < 3; ++px) {
            float v = bias;
            v = fmaf(xi[py][px], k0, v);
            v = fmaf(xi[py][px + 1], k1, v);
            v = fmaf(xi[py + 1][px], k2, v);
            v = fmaf(xi[py + 1][px + 1], k3, v);
            C1[(b * 9 + py * 3 + px) * C1S + ci] = f2bf_hw(fmaxf(v, 0.f));
          }
      }
    }
    // conv1 -> conv2 is wave-local: conv1 wrote C1 of images 8w .. 8w + 7, conv2's A fragments read images
    // b = 4 (2w + ii) + (fr >> 2), the same ones; W2 and CB2 were written behind the D load's barrier, KEEP behind the
    // B wait's (or the D wait's) barriers.  C1 is read by every wave in the backward (cfrag, c1v) and next written by
    // the next step's conv1: the barrier behind RED, the one in front of C's part 2, the C-publish barrier and the D
    // load's barrier lie between.  POOL / AM, written below, are published by the barrier in front of the fc1 partial
    // product, which stays: its A fragments read every image's POOL row
    wave_or_wg(HOPSX_WL_HAND(a) & HAND_WL_FWD);
    // ---- conv2 (MFMA, rows (b, q) = b*4 + q, k = tap*32 + ci) + bias + relu + max-pool + dropout ----
    // (one wave per SIMD: an LDS read that is waited for at once exposes its whole latency, so every phase below
    // issues its LDS reads in batches ahead of their uses — the fragments of MFMA step kk + 1 while step kk's MFMAs
    // issue, two register sets — and sched_barrier keeps the compiler from sinking them back next to the uses)
    {
      f32x4 acc[2][4];
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[ii][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      // the epilogue's operands (4 biases, 8 keep bytes), read ahead of the MFMA loop
      float bias[4];
      unsigned char keep[2][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bias[j] = CB2[j * 16 + fr];
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) keep[ii][j] = KEEP[(4 * (2 * w + ii) + fq) * C2 + j * 16 + fr];
      }
      bf16x8 af[2][2], bfr[2][4];
      auto frag = [&](int kk, int st) {
        const int di = kk >> 1, dj = kk & 1;
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) {
          const int b = 4 * (2 * w + ii) + (fr >> 2), q = fr & 3;
          const int pos = ((q >> 1) + di) * 3 + (q & 1) + dj;
          af[st][ii] = lds8(C1 + (b * 9 + pos) * C1S + fq * 8);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) bfr[st][j] = lds8(W2 + (j * 16 + fr) * W2S + kk * 32 + fq * 8);
      };
      frag(0, 0);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        if (kk + 1 < 4) frag(kk + 1, (kk + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int ii = 0; ii < 2; ++ii) acc[ii][j] = mma32(af[kk & 1][ii], bfr[kk & 1][j], acc[ii][j]);
      }
      bf16_raw pv[2][4];
      unsigned char av[2][4];
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float best = -INFINITY;
          int bi = 0;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float v = bf2f(f2bf_hw(fmaxf(acc[ii][j][r] + bias[j], 0.f)));  // bf16 conv output, as unfused
            if (v > best) {
              best = v;
              bi = r;
            }
          }
          if (!(best > 0.f)) bi = 0xFF;
          if (keep[ii][j]) {
            best *= inv;
          } else {
            best = 0.f;
            bi = 0xFF;
          }
          pv[ii][j] = f2bf_hw(best);
          av[ii][j] = (unsigned char)bi;
        }
      // (the stores after all the math: a store between two reads would be waited out with them)
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int b = 4 * (2 * w + ii) + fq, co = j * 16 + fr;
          POOL[b * PLS + co] = pv[ii][j];
          AM[b * C2 + co] = av[ii][j];
        }
    }
    __syncthreads();
    stamp(a, s, 1);
    // ---- fc1 partial product over this position's 64 inputs: part[b][n] ----
    {
      f32x4 acc[2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) acc[i][jj] = (f32x4){0.f, 0.f, 0.f, 0.f};
      bf16x8 af[2][2], bfr[2][2];  // both k steps' fragments in flight before the first MFMA
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int i = 0; i < 2; ++i) af[kk][i] = lds8(POOL + (i * 16 + fr) * PLS + kk * 32 + fq * 8);
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) bfr[kk][jj] = lds8(W1 + ((2 * w + jj) * 16 + fr) * W1S + kk * 32 + fq * 8);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) acc[i][jj] = mma32(af[kk][i], bfr[kk][jj], acc[i][jj]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
          for (int r = 0; r < 4; ++r) STG[(i * 16 + fq * 4 + r) * HID + (2 * w + jj) * 16 + fr] = acc[i][jj][r];
    }
    {  // publish A
      const auto R = rsrc(a.slabA + ((long)par * NPOS + p) * (B * HID));
      f32x4 v[4];  // every LDS read of the staging tile first, then the write-through stores
      if (HOPSX_WL_HAND(a) & HAND_WL_A) {
        // Wave w's accumulators are columns 32w .. 32w + 31 of all 32 rows: one whole 128-byte line per image.  It
        // reads them back itself — chunk c = lane + 64 k is row c >> 3, 16-byte piece c & 7 of its columns, so each
        // store instruction writes 8 whole lines — and stores without waiting for the other waves.  STG's first
        // 16 KB were last read by the previous step's C part 1, many barriers back; they are next written by the
        // conv2 weight gradient, behind the B wait's barrier, which every wave passes after this read-back
        wave_lds_order();
        int off[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int c = lane + 64 * k;
          off[k] = (c >> 3) * HID + 32 * w + (c & 7) * 4;
          v[k] = *(const f32x4*)(STG + off[k]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 4; ++k) bst16<SC1>(R, off[k] * 4, v[k]);
      } else {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = *(const f32x4*)(STG + (tid + 256 * k) * 4);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 4; ++k) bst16<SC1>(R, (tid + 256 * k) * 16, v[k]);
      }
      drain();
      __syncthreads();
      if (tid == 0) flag_store(a.flags + FL_A + p, ep);
    }
    const unsigned gep = (unsigned)(xs0 + s + 1);  // cross-rank epoch (grows across launches)
    if constexpr (DP) {
      // push this position's pooled activations to every peer, already in the fc1-wgrad B-fragment
      // layout (wave w: column block j = w; k = image), for the peers' fc1 weight gradient at the end
      // of the step; off the critical path (the peers read them after their conv backward)
      const int c0 = w * 16 + 4 * tp;
      const f32x4 f = __builtin_bit_cast(f32x4, lds_tr(POOL + (8 * fq + tq) * PLS + c0, POOL + (8 * fq + tq + 4) * PLS + c0));
      for (int r = 0; r < a.world; ++r) {
        if (r == a.rank) continue;
        bst16<SYS>(rsrc(a.xbuf[r] + XO_POOL + (par * XMAX + xslot(a, r)) * XS_POOL + (long)p * 4096), (w * 64 + lane) * 16, f);
      }
      // (flags raised after the B wait: by then the stores have long completed, so the drain is free)
    }
    if (s + 1 < a.nsteps) xv = xload(s + 1);  // next step's patch, consumed next iteration
    stamp(a, s, 2);
    // the next step's keep mask, at the head of the B wait: the heads need ~6 us from here, and KEEP was last read
    // by this step's conv2 epilogue, two barriers back (draw_keep writes other waves' images: the barrier in front of
    // the fc1 partial product and the one in the A publish between drain and flag; neither is one HAND_WL_* removes)
    if ((a.hand & HAND_FILL_KEEP) && s + 1 < a.nsteps) draw_keep(s + 1);
    // ---- B: dh of all 32 images ----
    // (step 0: the heads run on this GPU only, so a B that has not come within tmo0 means workgroups of
    // this launch are not resident — fail fast with the co-residency code instead of waiting out tmo)
    if (a.hand & 1) {
      // tagged form: the heads' {bf16 dh pair, epoch} granules are the flag.  Wave 0 gates on one granule per
      // head, then every thread sweeps its 8 granules straight into DH: no flag poll, no barrier between
      // poll and load, no second L2 round trip, no fp32 -> bf16 conversion (the head made the same bits)
      const unsigned long long* TB = (const unsigned long long*)(a.flags + FL_WORDS) + par * TGB_N;
      const unsigned code = s ? ecode(2, s) : ecode(12, 0);
      const long long tmo = s ? a.tmo : a.tmo0;
      if (!gate_tags(TB, p & (HID / 2 - 1), ep, (a.hand >> 8) & 0xFF, a.err, code, s_ok, tmo)) return;
      if (!sweep_tags<TGB_N / 256>(TB, tid, ep, a.err, code, s_ok + 2, tmo, [&](int idx, unsigned v) {
            *(unsigned*)(DH + (idx >> 6) * DHS + 2 * (idx & 63)) = v;
          }))
        return;
      if constexpr (DP) {
        drain();
        __syncthreads();
        if (tid < 64) raise_peers(a, XF_POOL + p, NPOS, gep);
      }
      stamp(a, s, 3);  // (the dh load is inside the wait in this form)
    } else {
    if (!wait_all(a.flags + FL_B, NHEAD, ep, a.err, s ? ecode(2, s) : ecode(12, 0), a.acquire, s_ok,
                  s ? a.tmo : a.tmo0, a.pollw_b, a.stagger, (a.hand & 2)))
      return;
    if constexpr (DP) {
      drain();
      __syncthreads();
      if (tid < 64) raise_peers(a, XF_POOL + p, NPOS, gep);
    }
    stamp(a, s, 3);
    {
      const auto R = rsrc(a.slabB + (long)par * NHEAD * PAY);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int idx = tid + 256 * k, b = idx >> 5, n4 = idx & 31;
        const f32x4 v = bld16<SC1>(R, (b * PAY + PAY_DH + n4 * 4) * 4);
        *(bf16x4*)(DH + b * DHS + n4 * 4) =
            (bf16x4){(short)f2bf_hw(v[0]), (short)f2bf_hw(v[1]), (short)f2bf_hw(v[2]), (short)f2bf_hw(v[3])};
      }
    }
    __syncthreads();
    }
    // ---- fc1 input gradient ----
    f32x4 gw[2][4], dp[2];
    // The fc1 slice update (Adadelta on the lane-owned registers, new bf16 weights for the next forward) in NFCH
    // chunks, c static: chunk c is elements c FCH .. c FCH + FCH - 1 of the whole update's order (ii, j, r).  fleft
    // (wave-uniform) holds the chunks not yet run this step: each runs exactly once, inside the owners' C wait or,
    // whatever is left, where the whole update has always run, behind the D publish
    auto fc1_chunk = [&](int c) {
#pragma unroll
      for (int q = 0; q < FCH; ++q) {
        const int el = c * FCH + q, ii = el >> 4, j = (el >> 2) & 3, r = el & 3;
        wm[ii][j][r] = adadelta(wm[ii][j][r], gw[ii][j][r] * hp.gscale, g1[ii][j][r], g2[ii][j][r], hp);
        W1[((2 * w + ii) * 16 + fq * 4 + r) * W1S + j * 16 + fr] = f2bf_hw(wm[ii][j][r]);
      }
    };
    unsigned fleft = (1u << NFCH) - 1u;
    unsigned char amv[2][4];  // the pool backward's argmax bytes, read with the fragments
    const bool wlb = HOPSX_WL_HAND(a) & HAND_WL_BWD;
    {
      // every fragment and the 8 argmax bytes in flight before the first MFMA
      // (the weight gradient, which only the Adadelta at the end of the step needs, is computed behind the
      // first part of the C publish below: everything up to that publish is on the step's critical path)
      bf16x8 da[4][2], db4[4];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {  // A = dh (row b, k = n), B = W1^T (col co, k = n)
        const int k1 = kk * 32 + 8 * fq + tq;
        db4[kk] = lds_tr(W1 + k1 * W1S + w * 16 + 4 * tp, W1 + (k1 + 4) * W1S + w * 16 + 4 * tp);
#pragma unroll
        for (int i = 0; i < 2; ++i) da[kk][i] = lds8(DH + (i * 16 + fr) * DHS + kk * 32 + fq * 8);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) amv[i][r] = AM[(i * 16 + fq * 4 + r) * C2 + w * 16 + fr];
      __builtin_amdgcn_sched_barrier(0);
      dp[0] = dp[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int i = 0; i < 2; ++i) dp[i] = mma32(da[kk][i], db4[kk], dp[i]);
    }
    // (no barrier: the phases up to the fc1 Adadelta write neither DH, POOL nor W1)
    // ---- dropout / max-pool / relu backward -> dconv2[(b,q)][co]; conv2 bias gradient ----
    {
      const int co = w * 16 + fr;
      float db = 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int b = i * 16 + fq * 4 + r;
          const int am = amv[i][r];
          const bf16_raw gb = am != 0xFF ? f2bf_hw(dp[i][r] * inv) : (bf16_raw)0;
          db += bf2f(gb);
          // the image's 4 window taps are adjacent columns of row co: one 8-byte store
          *(bf16x4*)(DC2 + co * DCS + b * 4) = (bf16x4){(short)(am == 0 ? gb : 0), (short)(am == 1 ? gb : 0),
                                                        (short)(am == 2 ? gb : 0), (short)(am == 3 ? gb : 0)};
        }
      db += __shfl_xor(db, 16, 64);
      db += __shfl_xor(db, 32, 64);
      if (fq == 0) STG[OFF_B2 + co] = db;
    }
    // ---- conv2 weight gradient: dW2[co][(t,ci)] = sum_(b,q) dconv2[(b,q)][co] im2col[(b,q)][(t,ci)] ----
    {
      f32x4 acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      // k = kk*32 + 8*fq + tq is image b1 = kk*8 + 2*fq, window tap q1 = tq (k + 4 = image b1 + 1, same q): a
      // step's 8 im2col fragments sit at compile-time offsets from one base address per lane
      const bf16_raw* cb = C1 + (2 * fq * 9 + (tq >> 1) * 3 + (tq & 1)) * C1S + 4 * tp;
      bf16x8 af[2], bfr[2][8];
      auto cfrag = [&](int kk, int st) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int t = j >> 1;
          const bf16_raw* q = cb + (kk * 8 * 9 + (t >> 1) * 3 + (t & 1)) * C1S + (j & 1) * 16;
          bfr[st][j] = lds_tr(q, q + 9 * C1S);
        }
      };
      auto afrag = [&](int kk, int st) { af[st] = lds8(DC2 + (w * 16 + fr) * DCS + kk * 32 + fq * 8); };
      // Pool backward -> this weight gradient is wave-local: the pool backward wrote DC2 rows co = 16w + fr, afrag
      // reads rows 16w + fr.  DC2 was last read across waves by the previous step's conv2 input gradient, many
      // barriers back; this step's reads it behind the one workgroup barrier of the backward, below.  C1 is stable
      // since the forward, STG[OFF_B2 + co] is read behind the barrier in front of C's part 2
      if (wlb) wave_lds_order();
      cfrag(0, 0);  // (C1 is this step's conv1 output: readable ahead of the barrier that publishes DC2)
      if (!wlb) __syncthreads();
      stamp(a, s, 4);
      afrag(0, 0);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        if (kk + 1 < 4) {
          afrag(kk + 1, (kk + 1) & 1);
          cfrag(kk + 1, (kk + 1) & 1);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = mma32(af[kk & 1], bfr[kk & 1][j], acc[j]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) STG[(w * 16 + fq * 4 + r) * 128 + j * 16 + fr] = acc[j][r];
      if (wlb) {
        // publish C, part 1, per wave: its accumulators are STG rows 16w .. 16w + 15, 8 KB contiguous in the slabC
        // row.  It reads them back itself (chunk lane + 64 k: each store instruction writes 8 whole lines) and stores
        // as soon as its own MFMAs are done, ahead of the backward's one barrier.  These rows of STG are next
        // written by the next step's fc1 partial product, many barriers on
        wave_lds_order();
        const auto R = rsrc(a.slabC + ((long)par * NPOS + p) * NCONV);
        constexpr int NK = OFF_B2 / 4 / 256;
        f32x4 v[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) v[k] = *(const f32x4*)(STG + (w * (64 * NK) + lane + 64 * k) * 4);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < NK; ++k) bst16<SC1>(R, (w * (64 * NK) + lane + 64 * k) * 16, v[k]);
      }
    }
    // ---- conv2 input gradient -> col2im -> relu' -> conv1 weight / bias gradient ----
    {
      const int mh = w >> 1, h = w & 1, ci = h * 16 + fr;
      // without HAND_WL_BWD both k steps' fragments are read ahead of the barrier below (DC2 and W2 are
      // stable there), so they arrive while the publish's staging reads and stores issue
      bf16x8 af[2][4], bfr[2][4];
      auto dfrag = [&]() {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int k1 = kk * 32 + 8 * fq + tq;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int m0 = (mh * 4 + i) * 16 + 4 * tp;
            af[kk][i] = lds_tr(DC2 + k1 * DCS + m0, DC2 + (k1 + 4) * DCS + m0);
          }
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int c0 = (2 * t + h) * 16 + 4 * tp;
            bfr[kk][t] = lds_tr(W2 + k1 * W2S + c0, W2 + (k1 + 4) * W2S + c0);
          }
        }
      };
      // The transposed DC2 reads cross waves (every row co, written by wave co >> 4).  Without HAND_WL_BWD the barrier
      // in front of the weight gradient published DC2 and this one the staging tile; with it this is the backward's
      // ONE workgroup barrier: DC2 is read behind it, and C's part 1 has left ahead of it
      // (one copy of the reads, a barrier on either side of it: with the reads in both arms of a branch the compiler
      // kept both sets of 64 registers and the data-parallel instantiation spilled)
      if (wlb) __syncthreads();
      dfrag();
      if (!wlb) {
        __syncthreads();
        // publish C, part 1: the conv2 weight gradient (8192 floats) now; its write-through stores drain
        // while the conv2 input gradient and the conv1 gradient below are computed
        const auto R = rsrc(a.slabC + ((long)par * NPOS + p) * NCONV);
        constexpr int NK = OFF_B2 / 4 / 256;
        f32x4 v[NK];  // every LDS read of the staging tile first, then the write-through stores
#pragma unroll
        for (int k = 0; k < NK; ++k) v[k] = *(const f32x4*)(STG + (tid + 256 * k) * 4);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < NK; ++k) bst16<SC1>(R, (tid + 256 * k) * 16, v[k]);
      }
      f32x4 acc[4][4];  // [M tile mh*4+i][tap t (N tile 2t+h)]
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[i][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[i][t] = mma32(af[kk][i], bfr[kk][t], acc[i][t]);
      // relu' of conv1: the 36 conv1 outputs of this lane's (b, ci), all in flight while the MFMAs run
      bf16_raw c1v[4][9];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int pos = 0; pos < 9; ++pos) c1v[i][pos] = C1[((4 * (mh * 4 + i) + fq) * 9 + pos) * C1S + ci];
      // ---- fc1 weight gradient (lane-owned layout), off the critical path: the C publish is draining ----
      // data parallel: the weight gradient sums every replica's images in rank order at the end of
      // the step (below)
      if constexpr (!DP) {
        bf16x8 wa[2], wb[4];
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) {  // A = dh^T (row n, k = b)
          const int n0 = (2 * w + ii) * 16 + 4 * tp;
          wa[ii] = lds_tr(DH + (8 * fq + tq) * DHS + n0, DH + (8 * fq + tq + 4) * DHS + n0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // B = pooled (col co, k = b)
          const int c0 = j * 16 + 4 * tp;
          wb[j] = lds_tr(POOL + (8 * fq + tq) * PLS + c0, POOL + (8 * fq + tq + 4) * PLS + c0);
        }
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
          for (int j = 0; j < 4; ++j) gw[ii][j] = mma32(wa[ii], wb[j], (f32x4){0.f, 0.f, 0.f, 0.f});
      }
      float gk[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
      f32x4 xq[2][4];  // image b's 4x4 input patch, read one image ahead of its use
#pragma unroll
      for (int c = 0; c < 4; ++c) xq[0][c] = *(const f32x4*)(XIN + (4 * (mh * 4) + fq) * 16 + 4 * c);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i + 1 < 4) {
#pragma unroll
          for (int c = 0; c < 4; ++c) xq[(i + 1) & 1][c] = *(const f32x4*)(XIN + (4 * (mh * 4 + i + 1) + fq) * 16 + 4 * c);
        }
        float d[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) d[k] = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int q = 0; q < 4; ++q) d[((q >> 1) + (t >> 1)) * 3 + (q & 1) + (t & 1)] += acc[i][t][q];
        const f32x4* xi = xq[i & 1];
#pragma unroll
        for (int py = 0; py < 3; ++py)
#pragma unroll
          for (int px = 0; px < 3; ++px) {
            const int pos = py * 3 + px;
            const float dd = (short)c1v[i][pos] > 0 ? d[pos] : 0.f;  // relu' of conv1
            gk[0] = fmaf(dd, xi[py][px], gk[0]);
            gk[1] = fmaf(dd, xi[py][px + 1], gk[1]);
            gk[2] = fmaf(dd, xi[py + 1][px], gk[2]);
            gk[3] = fmaf(dd, xi[py + 1][px + 1], gk[3]);
            gk[4] += dd;
          }
      }
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        gk[k] += __shfl_xor(gk[k], 16, 64);
        gk[k] += __shfl_xor(gk[k], 32, 64);
      }
      if (fq == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) RED[(mh * 32 + ci) * 5 + k] = gk[k];
      }
    }
    __syncthreads();
    if (tid < 32 * 5) {
      const int ci = tid / 5, k = tid - ci * 5;
      const float v = RED[ci * 5 + k] + RED[(32 + ci) * 5 + k];
      if (k < 4) STG[OFF_W1 + ci * 4 + k] = v;
      else STG[OFF_B1 + ci] = v;
    }
    __syncthreads();
    stamp(a, s, 5);
    {  // publish C, part 2: the 224 small gradients [b2 | conv1 w | conv1 b]; every wave drains both parts
      const auto R = rsrc(a.slabC + ((long)par * NPOS + p) * NCONV);
      const int idx = OFF_B2 / 4 + tid;
      if (idx < NCONV / 4) bst16<SC1>(R, idx * 16, *(const f32x4*)(STG + idx * 4));
      drain();
      __syncthreads();
      if (tid == 0) flag_store(a.flags + FL_C + p, ep);
    }
    stamp(a, s, 6);
    // ---- slice owners: fixed-order reduce of 64 params over the 169 partials, Adadelta, publish D ----
    if (owner) {
      const int e0 = p * SLICE;
      // Item (g, j): quad j (16 bytes) of the slice's row in the partials pp = g + 19 k of group g, k < 9, summed in
      // that order into RED[g].  Wave w holds groups 4w .. 4w + 3, 16 lanes each (thread = 16 g + j), so one wave
      // instruction reads 4 whole rows of the slice (2 whole 128-byte lines each) and nothing else; groups 16 .. 18
      // are a second item (rows 9 .. 17 of the thread) on the last 16 lanes of waves 0 .. 2, in flight with the
      // first.  A row past the end of the slice (slice 131 is half filled) is not loaded: RED gets its zeros
      const int j = lane & (NQ - 1), lq = lane >> 4, g = 4 * w + lq, gx = 16 + w;
      const bool act = e0 + 4 * j < NCONV, two = lq == 3 && gx < NRED;
      const auto R = rsrc(a.slabC + (long)par * NPOS * NCONV);
      f32x4 v[2 * NKC];
#pragma unroll
      for (int k = 0; k < 2 * NKC; ++k) v[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
      auto load = [&](int k) {
        const int pp = k < NKC ? g + NRED * k : gx + NRED * (k - NKC);
        v[k] = bld16<SC1>(R, (pp * NCONV + e0 + 4 * j) * 4);
      };
      // the rows this thread loads: all 9 of its first group (g < 16), and of the second the 9 or 8 that exist
      const unsigned rows2 = gx + NRED * (NKC - 1) < NPOS ? (1u << NKC) - 1u : (1u << (NKC - 1)) - 1u;
      const unsigned pend = !act ? 0u : ((1u << NKC) - 1u) | (two ? rows2 << NKC : 0u);
      bool lost = false;  // the flag form's wait gave up (uniform)
      if ((a.hand & 8) && !a.acquire) {
        // progressive form (HOPSX_PERSIST_PROG bit 1): the rows are loaded as their flags arrive.  Lane l < 36 of
        // wave w polls the flag of group 4w + l / 9, partial k = l % 9, lanes 36 .. 44 of waves 0 .. 2 those of
        // group 16 + w: bit 9 lq + k of the ballot is this thread's row k, and for the threads with a second item
        // (lq = 3) bits 36 .. 44 follow as its rows 9 .. 17
        const int lp = lane < 4 * NKC ? 4 * w + lane / NKC + NRED * (lane % NKC) : gx + NRED * (lane - 4 * NKC);
        const bool mine = lane < 4 * NKC || (gx < NRED && lane < 5 * NKC && lp < NPOS);
        // the fill (HAND_FILL_C, <false> only: the data-parallel weight gradient does not exist yet): this wave's
        // next chunk of the fc1 update per poll, up to the cap; the chunk index selects among statically indexed
        // copies (the pend-mask idiom), so wm / g1 / g2 / gw stay in registers
        int fcap = !DP && (a.hand & HAND_FILL_C) ? (a.hand >> HAND_FMAX_SHIFT) & 15 : 0;
        auto fill = [&]() -> bool {
          if (fcap <= 0) return false;
          // (fcap <= NFCH: a chunk is left; wave-uniform, and told so: scalar branches around the copies)
          const unsigned bit = __builtin_amdgcn_readfirstlane(fleft & (0u - fleft));
#pragma unroll
          for (int c = 0; c < NFCH; ++c)
            if ((bit >> c) & 1u) fc1_chunk(c);
          fleft &= ~bit;
          --fcap;
          return true;
        };
        gather_rows<2 * NKC>(a.flags + FL_C + lp, mine, lq * NKC, pend, ep, a.err, ecode(3, s), s_ok + 2, a.tmo, load,
                             fill);
        stamp(a, s, 7);  // (the partials' load is inside the wait in this form)
      } else {
        lost = !wait_all(a.flags + FL_C, NPOS, ep, a.err, ecode(3, s), a.acquire, s_ok, a.tmo, a.pollw_c, a.stagger,
                         (a.hand & 2));
        stamp(a, s, 7);
#pragma unroll
        for (int k = 0; k < 2 * NKC; ++k)  // every row in flight before the sum
          if (!lost && ((pend >> k) & 1u)) load(k);
      }
      // every lane names its partial registers here, on EVERY path out of the two forms (a lost wait leaves below,
      // behind the sum), so the compiler waits for the loads here, where the sum's lanes wait anyway.  On a path
      // around this use its bookkeeping keeps them pending and waits vmcnt(0) where those registers are next
      // written: that landed behind the D flag store, and wave 0 waited out the store's round trip (0.5 - 0.7 us)
      // before its fc1 Adadelta (seen twice: a conditional sum, and an early return of the flag form)
#pragma unroll
      for (int k = 0; k < 2 * NKC; ++k) asm volatile("" ::"v"(v[k]));
      {
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NKC; ++k) acc += v[k];
        *(f32x4*)(RED + g * SLICE + 4 * j) = acc;
      }
      if (two) {
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NKC; ++k) acc += v[NKC + k];
        *(f32x4*)(RED + gx * SLICE + 4 * j) = acc;
      }
      __syncthreads();
      {
        const int f = s_ok[2];  // (a wave of the progressive gather gave up)
        if (lost || f) return;
      }
      const int e = e0 + tid;
      float gs = 0.f;
      if (tid < SLICE) {
        for (int g = 0; g < NRED; ++g) gs += RED[g * SLICE + tid];
      }
      if constexpr (DP) {
        // this rank's slice sum to every peer, then every replica's, summed in rank order (identical
        // on every rank, so the replicas stay bit-identical)
        if (tid < 64) {
          if (tid < SLICE) {
            for (int r = 0; r < a.world; ++r) {
              if (r == a.rank) continue;
              bst4<SYS>(rsrc(a.xbuf[r] + XO_CONV + (par * XMAX + xslot(a, r)) * XS_CONV), e * 4, gs);
            }
          }
          drain();
          raise_peers(a, XF_CONV + p, NSLICE, gep);
        }
        if (!wait_peers(a, XF_CONV + p, NSLICE, gep, ecode(6, s), s_ok)) return;
        if (tid < SLICE) {
          const auto X = rsrc(a.xbuf[a.rank] + XO_CONV + (long)par * XMAX * XS_CONV);
          float v[XMAX];  // every peer's value in flight before the rank-order sum
#pragma unroll
          for (int r = 0; r < XMAX; ++r) v[r] = r < a.world && r != a.rank ? bld4<SYS>(X, (int)(r * XS_CONV) + e * 4) : gs;
          float t = 0.f;
#pragma unroll
          for (int r = 0; r < XMAX; ++r)
            if (r < a.world) t += v[r];
          gs = t;
        }
      }
      if (w == 0) {  // one full wave: lane = element of the slice (SLICE == 64)
        float wn = 0.f;
        if (e < NCONV) {
          SLm[tid] = adadelta(SLm[tid], gs * hp.gscale, SL1[tid], SL2[tid], hp);
          wn = SLm[tid];
        }
        // the D payload, whole 128-byte lines written by ONE store instruction of this wave (4-byte write-through
        // sc1 stores): an owner of conv2 weights its line of 64 bf16 (pairs, the even lanes), the four owners of
        // the small parameters their two lines of fp32 (slice 131: one, it is half filled)
        const float wnext = __shfl_down(wn, 1, 64);
        unsigned char* D = (unsigned char*)a.slabD + (long)par * D_BYTES;
        if (p < OFF_B2 / SLICE) {
          if (!(lane & 1))
            __hip_atomic_store((gu32*)(D + e * 2), (unsigned)f2bf_hw(wn) | ((unsigned)f2bf_hw(wnext) << 16),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (e < NCONV) {
          __hip_atomic_store((gu32*)(D + D_F32 + (e - OFF_B2) * 4), __float_as_uint(wn), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
        }
        drain();
        if (lane == 0) flag_store(a.flags + FL_D + p, ep);
      }
      stamp(a, s, 8);
    }
    if constexpr (DP) {
      // ---- fc1 weight gradient over every replica's images: dh^T fragments (each rank's head 0) and
      // pooled fragments (each rank's position p); one MFMA product per replica, summed in rank order
      // (the per-replica gradients, added exactly as an all-reduce in rank order would).  After the
      // owner phase: placed before the owners' C wait it delayed the D publish (measured +2 us at 8
      // loopback ranks: the exchange-buffer loads take longer than that wait) ----
      if (!wait_peers(a, XF_H, 1, gep, ecode(7, s), s_ok)) return;
      if (!wait_peers(a, XF_POOL + p, NPOS, gep, ecode(8, s), s_ok)) return;
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int j = 0; j < 4; ++j) gw[ii][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      const auto XP = rsrc(a.xbuf[a.rank] + XO_POOL + (long)par * XMAX * XS_POOL + (long)p * 4096);
      const auto XD = rsrc(a.xbuf[a.rank] + XO_DHT + (long)par * XMAX * XS_DHT);
      // rank r's fragments: own from LDS, a peer's from this rank's exchange buffer; loaded two ranks
      // ahead of the MFMAs that consume them (three register sets, indices fixed by the unrolled loop;
      // four — three peers' loads in flight — measured no faster at 8 loopback ranks: 34.2 vs 33.6 us/step)
      constexpr int PF = 3;
      bf16x8 af[PF][2], bfr[PF][4];
      auto fetch = [&](int r, int b) {
        if (r == a.rank) {
#pragma unroll
          for (int ii = 0; ii < 2; ++ii) {
            const int n0 = (2 * w + ii) * 16 + 4 * tp;
            af[b][ii] = lds_tr(DH + (8 * fq + tq) * DHS + n0, DH + (8 * fq + tq + 4) * DHS + n0);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c0 = j * 16 + 4 * tp;
            bfr[b][j] = lds_tr(POOL + (8 * fq + tq) * PLS + c0, POOL + (8 * fq + tq + 4) * PLS + c0);
          }
        } else {
#pragma unroll
          for (int ii = 0; ii < 2; ++ii)
            af[b][ii] = __builtin_bit_cast(bf16x8, bld16<SYS>(XD, (int)(r * XS_DHT) + ((2 * w + ii) * 64 + lane) * 16));
#pragma unroll
          for (int j = 0; j < 4; ++j)
            bfr[b][j] = __builtin_bit_cast(bf16x8, bld16<SYS>(XP, (int)(r * XS_POOL) + (j * 64 + lane) * 16));
        }
      };
#pragma unroll
      for (int r = 0; r < PF - 1; ++r)
        if (r < a.world) fetch(r, r);
#pragma unroll
      for (int r = 0; r < XMAX; ++r) {
        if (r < a.world) {
          if (r + PF - 1 < XMAX && r + PF - 1 < a.world) fetch(r + PF - 1, (r + PF - 1) % PF);
#pragma unroll
          for (int ii = 0; ii < 2; ++ii)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              gw[ii][j] += mma32(af[r % PF][ii], bfr[r % PF][j], (f32x4){0.f, 0.f, 0.f, 0.f});
        }
      }
    }
    // ---- Adadelta on the fc1 slice (registers) and the new bf16 weights for the next forward: off the
    // critical path, while this workgroup waits for the D hand-off (W1 is next read after it).  The owners of
    // <false> have run some or all of its chunks inside their C wait: here whatever is left ----
#pragma unroll
    for (int c = 0; c < NFCH; ++c)
      if ((__builtin_amdgcn_readfirstlane(fleft) >> c) & 1u) fc1_chunk(c);
    // (KEEP is next read after the D wait's barrier)
    if (!(a.hand & HAND_FILL_KEEP) && s + 1 < a.nsteps) draw_keep(s + 1);
    stamp(a, s, 9);
    // ---- D: the updated conv parameters for the next step ----
    if (!owner && tid < 64) {
      // The NPOS - NSLICE positions that own no slice get here ~5 us before the owners publish.  Polling every flag
      // line all that time delays the owners' flag stores to those lines (last D publish -> D ready 1.1 -> 1.8 us
      // for the earliest position with 37 such pollers instead of 7, profiles/r15_persist_aligned_slices.txt).  So
      // they first watch ONE line, the flags of the four owners of the small parameters, from four lanes; the gate
      // only delays the wait below, which checks every flag and the error word: it is bounded by time alone
      constexpr int G0 = OFF_B2 / SLICE;
      const bool mine = lane < NSLICE - G0;
      const long long t0 = wall_clock64();
      for (;;) {
        const unsigned f = mine ? flag_load(a.flags + FL_D + G0 + lane) : ep;
        if (__all(f == ep) || wall_clock64() - t0 > 2000) break;  // (20 us: far longer than the owners' phase)
        __builtin_amdgcn_s_sleep(4);
      }
    }
    if (!wait_all(a.flags + FL_D, NSLICE, ep, a.err, ecode(4, s), a.acquire, s_ok, a.tmo, a.pollw_d, a.stagger,
                  (a.hand & 2)))
      return;
    stamp(a, s, 10);
    {
      const auto R = rsrc((const unsigned char*)a.slabD + (long)par * D_BYTES);
      constexpr int NB = OFF_B2 * 2 / 16;        // 1024 16-B chunks of bf16 conv2 weights
      constexpr int NF = (NCONV - OFF_B2) / 4;   // 56 16-B chunks of fp32
      f32x4 dv[NB / 256 + 1];
#pragma unroll
      for (int k = 0; k < NB / 256; ++k) dv[k] = bld16<SC1>(R, (tid + 256 * k) * 16);
      dv[NB / 256] = tid < NF ? bld16<SC1>(R, D_F32 + tid * 16) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < NB / 256; ++k) {
        const int c = tid + 256 * k;  // chunk c: conv2 row c >> 4, 8 values from column (c & 15) * 8
        *(f32x4*)(W2 + (c >> 4) * W2S + (c & 15) * 8) = dv[k];
      }
      if (tid < NF) {
        const int j = OFF_B2 + tid * 4;  // 4 params never straddle a region (8256, 8384 are multiples of 4)
        float* dst = j < OFF_W1 ? CB2 + (j - OFF_B2) : (j < OFF_B1 ? CW1 + (j - OFF_W1) : CB1 + (j - OFF_B1));
        *(f32x4*)dst = dv[NB / 256];
      }
    }
    __syncthreads();
    stamp(a, s, 11);
  }

  // ---- write back: fc1 slice and the owned conv slice (master, state, bf16 shadow) ----
#pragma unroll
  for (int ii = 0; ii < 2; ++ii)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = (2 * w + ii) * 16 + fq * 4 + r, co = j * 16 + fr;
        const long ai = a.off[4] + (long)n * KIN + p * C2 + co;
        a.master[ai] = wm[ii][j][r];
        a.s1[ai] = g1[ii][j][r];
        a.s2[ai] = g2[ii][j][r];
        a.shadow[ai] = f2bf_hw(wm[ii][j][r]);
      }
  if (owner && tid < SLICE) {
    const int e = p * SLICE + tid;
    if (e < NCONV) {
      const long ci = conv_idx(a, e);
      a.master[ci] = SLm[tid];
      a.s1[ci] = SL1[tid];
      a.s2[ci] = SL2[tid];
      a.shadow[ci] = f2bf_hw(SLm[tid]);
    }
  }
  stamp(a, a.nsteps - 1, 14);  // (debug stamps: write-back issued)
  // every workgroup has started (D of the last step needs C of every position, which needs B of
  // every head): the run-state words can advance
  if (p == 0 && tid == 0) {
    if constexpr (DP) a.xstep[0] = xs0 + a.nsteps;
    a.cursor[0] = (cur0 + a.nsteps) % a.nbatch;
    *(unsigned long long*)(a.flags + FL_EPOCH) = eb + (unsigned long long)a.nsteps;
    a.rng[1] = ctr0 + (unsigned long long)a.nsteps;
    if (a.step_dev) a.step_dev[0] += (float)a.nsteps;
  }
}

// ------------------------------------------------------------------------------------------------
// head workgroup i (image i): fc1 reduce + bias + relu, Dense10, softmax CE, dh; replicated
// fc2 / fc1-bias Adadelta from all 32 payloads
// ------------------------------------------------------------------------------------------------
template <bool DP>
__device__ __forceinline__ void head_wg(const Args& a, unsigned char* smem, int* s_ok, const OptHP& hp,
                                        long long cur0, long long xs0, unsigned long long eb) {
  const int i = blockIdx.x - NPOS;
  const int tid = threadIdx.x, lane = tid & 63;
  float* HW = (float*)(smem + H_W2);
  float* HW1 = HW + NCLS * HID;
  float* HW2 = HW1 + NCLS * HID;
  float* HB2 = (float*)(smem + H_B2);  // [0,16) master [16,32) s1 [32,48) s2
  float* HB1 = (float*)(smem + H_B1);  // [0,128) master [128,256) s1 [256,384) s2
  float* RED = (float*)(smem + H_RED);
  float* HH = (float*)(smem + H_H);
  float* LOG = (float*)(smem + H_LOG);
  float* PAYL = (float*)(smem + H_PAY);
  float* ALL = (float*)(smem + H_ALL);
  {
    constexpr int NJ = NCLS * HID / 256;  // (all loads in flight before the LDS stores)
    float v0[NJ], v1[NJ], v2[NJ];
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
      const long ai = a.off[6] + tid + 256 * q;
      v0[q] = a.master[ai];
      v1[q] = a.s1[ai];
      v2[q] = a.s2[ai];
    }
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
      HW[tid + 256 * q] = v0[q];
      HW1[tid + 256 * q] = v1[q];
      HW2[tid + 256 * q] = v2[q];
    }
  }
  if (tid < NCLS) {
    const long ai = a.off[7] + tid;
    HB2[tid] = a.master[ai];
    HB2[16 + tid] = a.s1[ai];
    HB2[32 + tid] = a.s2[ai];
  }
  if (tid < HID) {
    const long ai = a.off[5] + tid;
    HB1[tid] = a.master[ai];
    HB1[128 + tid] = a.s1[ai];
    HB1[256 + tid] = a.s2[ai];
  }
  if (tid == 0) {
    PAYL[266] = PAYL[267] = PAYL[270] = PAYL[271] = 0.f;
  }
  __syncthreads();

  for (int s = 0; s < a.nsteps; ++s) {
    const unsigned ep = (unsigned)(eb + (unsigned long long)s + 1ull);
    const int par = s & 1;
    const int y = (int)a.ys[((cur0 + s) % a.nbatch) * B + i];
    // The one-wave head's operands: lane l's two fc1 biases, its two columns of the fc2 weight, the ten fc2 biases.
    // They are stable from the barrier that closes the previous step's fc2 update (step 0: the prologue's) to this
    // step's update, so with HAND_HEAD_REGS they are read here, where the head waits for A anyway, and not inside
    // the chain from the last A flag to the granule store that releases the positions; the dh loop reads the
    // same registers.  (Opaque to the compiler behind the read, or it re-reads LDS at the use)
    float rb1[2], rw[NCLS][2], rb2[NCLS];
    auto head_operands = [&]() {
      const int n0 = 2 * lane;
#pragma unroll
      for (int u = 0; u < 2; ++u) rb1[u] = HB1[n0 + u];
#pragma unroll
      for (int c = 0; c < NCLS; ++c) {
#pragma unroll
        for (int u = 0; u < 2; ++u) rw[c][u] = HW[c * HID + n0 + u];
        rb2[c] = HB2[c];
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) asm volatile("" : "+v"(rb1[u]));
#pragma unroll
      for (int c = 0; c < NCLS; ++c) asm volatile("" : "+v"(rw[c][0]), "+v"(rw[c][1]), "+v"(rb2[c]));
    };
    if (tid < 64 && a.head1w && (a.hand & HAND_HEAD_REGS)) head_operands();  // (wave 0 alone computes the head)
    // ---- A: reduce the 169 fc1 partial rows of image i (fixed order) ----
    // On one GPU a head gets here ~9 us before the last position publishes A, and 32 heads polling all NLINE_A
    // flag lines at s_sleep(1) cadence all that time sit on the lines the 169 producers store their flags into (the
    // pattern that delayed the owners' D flag stores: the non-owners' gate at the end of position_wg).  So wave 0
    // first watches ONE line, a lane per flag, at a slow cadence, until the whole line carries the epoch
    // (HOPSX_PERSIST_GATE_A: 1 head i line i % NLINE_A, ~5 slow pollers a line; 2 every head line 0).  The gate
    // only delays the wait below, which checks every flag, the error word and the timeout as before; it is bounded
    // by time alone (gate_a_tk, also in step 0: a grid that is not co-resident fails gate_a_tk + tmo0 after entry).
    // It holds back wave 0 only: with HOPSX_PERSIST_POLLW_A > 1 the other polling waves enter the wait below at once
    // and poll every line at the fast cadence, so an A/B of POLLW_A measures the gate only at 1 (the default)
    if (const int ga = (a.hand >> HAND_GATEA_SHIFT) & 3; ga && tid < 64) {
      const int l0 = ga == 1 ? (i % NLINE_A) * 32 : 0;
      const bool mine = lane < 32 && l0 + lane < NPOS;
      const long long t0 = wall_clock64();
      for (;;) {
        const unsigned f = mine ? flag_load(a.flags + FL_A + l0 + lane) : ep;
        if (__all(f == ep) || wall_clock64() - t0 >= a.gate_a_tk) break;
        __builtin_amdgcn_s_sleep(4);
      }
    }
    if (!wait_all(a.flags + FL_A, NPOS, ep, a.err, s ? ecode(1, s) : ecode(12, 0), a.acquire, s_ok,
                  s ? a.tmo : a.tmo0, a.pollw_a, a.stagger, (a.hand & 2)))
      return;
    stamp(a, s, 0);
    {
      const int n4 = tid & 31, g = tid >> 5;
      const auto R = rsrc(a.slabA + (long)par * NPOS * B * HID);
      // all 22 loads in flight before the (fixed-order) sum: a load -> add chain serialises 22 L2 trips
      constexpr int NK = (NPOS + 7) / 8;
      f32x4 v[NK];
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int pp = g + 8 * k;
        v[k] = pp < NPOS ? bld16<SC1>(R, ((pp * B + i) * HID + n4 * 4) * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
      f32x4 acc = v[0];
#pragma unroll
      for (int k = 1; k < NK; ++k) acc += v[k];
      *(f32x4*)(RED + g * HID + n4 * 4) = acc;
    }
    __syncthreads();
    if (a.head1w) {
      // one wave does the whole head from registers (HOPSX_PERSIST_HEAD1W): lane l owns hidden units 2l,
      // 2l+1, the 10 logits are wave sums, softmax / dlogits / dh in registers, and the B payload leaves
      // as 8-B write-through stores from this wave alone (its drain then its flag: no barrier, no LDS
      // round trip) — four barriers and three LDS passes off the critical A -> B chain
      if (tid < 64) {
        const int n0 = 2 * lane;
        if (!(a.hand & HAND_HEAD_REGS)) head_operands();
        float h[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          float v = 0.f;
#pragma unroll
          for (int g = 0; g < 8; ++g) v += RED[g * HID + n0 + u];
          h[u] = fmaxf(v + rb1[u], 0.f);
        }
        // the ten logits: wave_sum_tree is wave_sum's pairing tree (the same bits) without its 6 LDS round trips
        float z[NCLS];
        if (a.hand & HAND_HEAD_TREE) {
#pragma unroll
          for (int c = 0; c < NCLS; ++c) z[c] = wave_sum_tree(fmaf(h[1], rw[c][1], h[0] * rw[c][0])) + rb2[c];
        } else {
#pragma unroll
          for (int c = 0; c < NCLS; ++c) z[c] = wave_sum(fmaf(h[1], rw[c][1], h[0] * rw[c][0])) + rb2[c];
        }
        float m = z[0];
#pragma unroll
        for (int c = 1; c < NCLS; ++c) m = fmaxf(m, z[c]);
        float e[NCLS], se = 0.f, zy = 0.f;
        int am = NCLS;
#pragma unroll
        for (int c = NCLS - 1; c >= 0; --c) {
          e[c] = __expf(z[c] - m);
          if (z[c] == m) am = c;  // the first maximum
          if (c == y) zy = z[c];
        }
#pragma unroll
        for (int c = 0; c < NCLS; ++c) se += e[c];
        const float inv_se = 1.f / se;
        float dl[NCLS];
#pragma unroll
        for (int c = 0; c < NCLS; ++c) dl[c] = (e[c] * inv_se - (c == y ? 1.f : 0.f)) * a.inv_gb;
        float dh[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          float d = 0.f;
#pragma unroll
          for (int c = 0; c < NCLS; ++c) d = fmaf(dl[c], rw[c][u], d);
          dh[u] = h[u] > 0.f ? d : 0.f;
        }
        // the tagged dh first (what the positions wait for): one 8-byte write-through store per lane, no drain
        // in front of it; the fp32 payload + flag below serve the heads' fc2 update and the DP push
        if (a.hand & 1)
          granule_store((unsigned long long*)(a.flags + FL_WORDS) + (par * NHEAD + i) * (HID / 2) + lane, ep,
                        (unsigned)f2bf_hw(dh[0]) | ((unsigned)f2bf_hw(dh[1]) << 16));
        const auto R = rsrc(a.slabB + ((long)par * NHEAD + i) * PAY);
        bst8<SC1>(R, (PAY_DH + n0) * 4, dh[0], dh[1]);
        bst8<SC1>(R, (PAY_H + n0) * 4, h[0], h[1]);
        float p0 = 0.f, p1 = 0.f;
#pragma unroll
        for (int c = 0; c < NCLS; c += 2)
          if (lane == c / 2) {
            p0 = dl[c];
            p1 = dl[c + 1];
          }
        if (lane < NCLS / 2) bst8<SC1>(R, (PAY_DL + 2 * lane) * 4, p0, p1);
        if (lane == NCLS / 2) bst8<SC1>(R, PAY_LOSS * 4, __logf(se) + m - zy, am == y ? 1.f : 0.f);
        drain();
        if (lane == 0) flag_store(a.flags + FL_B + i, ep);
      }
    }
    if (!a.head1w) {
    if (tid < HID) {
      float v = 0.f;
#pragma unroll
      for (int g = 0; g < 8; ++g) v += RED[g * HID + tid];
      HH[tid] = fmaxf(v + HB1[tid], 0.f);
    }
    __syncthreads();
    {  // logits: 16 lanes per class
      const int c = tid >> 4, part = tid & 15;
      float v = 0.f;
      if (c < NCLS) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v = fmaf(HH[part + 16 * k], HW[c * HID + part + 16 * k], v);
      }
      v = row_fold<1>(v);
      if (part == 0 && c < NCLS) LOG[c] = v + HB2[c];
    }
    __syncthreads();
    if (tid < 64) {  // softmax cross-entropy of image i (mean over the batch: 1/B)
      const float z = lane < NCLS ? LOG[lane] : -INFINITY;
      const float m = wave_max(z);
      const float e = lane < NCLS ? __expf(z - m) : 0.f;
      const float se = wave_sum(e);
      const unsigned long long hit = __ballot(lane < NCLS && z == m);
      const int am = __ffsll((long long)hit) - 1;
      if (lane < NCLS) PAYL[PAY_DL + lane] = (e / se - (lane == y ? 1.f : 0.f)) * a.inv_gb;
      if (lane == 0) {
        PAYL[PAY_LOSS] = __logf(se) + m - LOG[y];
        PAYL[PAY_COR] = am == y ? 1.f : 0.f;
      }
    }
    __syncthreads();
    if (tid < HID) {
      const float h = HH[tid];
      float d = 0.f;
#pragma unroll
      for (int c = 0; c < NCLS; ++c) d = fmaf(PAYL[PAY_DL + c], HW[c * HID + tid], d);
      PAYL[PAY_DH + tid] = h > 0.f ? d : 0.f;
      PAYL[PAY_H + tid] = h;
    }
    __syncthreads();
    {  // publish B (the tagged dh first, as in the one-wave form)
      if ((a.hand & 1) && tid < HID / 2)
        granule_store((unsigned long long*)(a.flags + FL_WORDS) + (par * NHEAD + i) * (HID / 2) + tid, ep,
                      (unsigned)f2bf_hw(PAYL[PAY_DH + 2 * tid]) | ((unsigned)f2bf_hw(PAYL[PAY_DH + 2 * tid + 1]) << 16));
      const auto R = rsrc(a.slabB + ((long)par * NHEAD + i) * PAY);
      if (tid < PAY / 4) bst16<SC1>(R, tid * 16, *(const f32x4*)(PAYL + tid * 4));
      drain();
      __syncthreads();
      if (tid == 0) flag_store(a.flags + FL_B + i, ep);
    }
    }
    stamp(a, s, 1);
    // ---- replicated fc2 / fc1-bias update from every image's payload ----
    if (!wait_all(a.flags + FL_B, NHEAD, ep, a.err, s ? ecode(5, s) : ecode(12, 0), a.acquire, s_ok,
                  s ? a.tmo : a.tmo0, a.pollw, a.stagger, (a.hand & 2)))
      return;
    {
      const auto R = rsrc(a.slabB + (long)par * NHEAD * PAY);
      constexpr int NK = (NHEAD * PAY / 4 + 255) / 256;
      f32x4 v[NK];
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int idx = tid + 256 * k;
        v[k] = idx < NHEAD * PAY / 4 ? bld16<SC1>(R, idx * 16) : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int idx = tid + 256 * k;
        if (idx < NHEAD * PAY / 4) *(f32x4*)(ALL + idx * 4) = v[k];
      }
    }
    __syncthreads();
    // this replica's fc2 / fc1-bias / fc2-bias gradients: element tid + 256 k of fc2.weight (k < 5),
    // fc1.bias[tid], fc2.bias[tid]
    constexpr int NW = NCLS * HID / 256;
    static_assert(NCLS * HID == NW * 256, "fc2 weight split");
    float gl[NW + 2];
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const int j = tid + 256 * k, c = j / HID, n = j - c * HID;
      float g = 0.f;
#pragma unroll 8
      for (int b = 0; b < B; ++b) g = fmaf(ALL[b * PAY + PAY_DL + c], ALL[b * PAY + PAY_H + n], g);
      gl[k] = g;
    }
    gl[NW] = gl[NW + 1] = 0.f;
    if (tid < HID) {
#pragma unroll 8
      for (int b = 0; b < B; ++b) gl[NW] += ALL[b * PAY + PAY_DH + tid];
    }
    if (tid < NCLS) {
      for (int b = 0; b < B; ++b) gl[NW + 1] += ALL[b * PAY + PAY_DL + tid];
    }
    if constexpr (DP) {
      const unsigned gep = (unsigned)(xs0 + s + 1);
      if (i == 0) {
        // head 0 pushes this replica's head gradients and dh^T (fc1-wgrad A fragments, bf16, the layout
        // the position workgroups read from their own LDS) to every peer
        bf16_raw* DS = (bf16_raw*)(smem + H_DHS);
        for (int e = tid; e < B * HID; e += 256) DS[(e >> 7) * DHS + (e & 127)] = f2bf_hw(ALL[(e >> 7) * PAY + PAY_DH + (e & 127)]);
        __syncthreads();
        const int w = tid >> 6, fr = lane & 15, fq = lane >> 4, tq = fr >> 2, tp = fr & 3;
        f32x4 fd[2];
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) {
          const int n0 = (2 * w + ii) * 16 + 4 * tp;
          fd[ii] = __builtin_bit_cast(f32x4, lds_tr(DS + (8 * fq + tq) * DHS + n0, DS + (8 * fq + tq + 4) * DHS + n0));
        }
        for (int r = 0; r < a.world; ++r) {
          if (r == a.rank) continue;
          const int sl = xslot(a, r);
          const auto XG = rsrc(a.xbuf[r] + XO_FC2 + (par * XMAX + sl) * XS_FC2);
#pragma unroll
          for (int k = 0; k < NW; ++k) bst4<SYS>(XG, (tid + 256 * k) * 4, gl[k]);
          if (tid < HID) bst4<SYS>(XG, (NCLS * HID + tid) * 4, gl[NW]);
          if (tid < NCLS) bst4<SYS>(XG, (NCLS * HID + HID + tid) * 4, gl[NW + 1]);
          const auto XD = rsrc(a.xbuf[r] + XO_DHT + (par * XMAX + sl) * XS_DHT);
#pragma unroll
          for (int ii = 0; ii < 2; ++ii) bst16<SYS>(XD, ((2 * w + ii) * 64 + lane) * 16, fd[ii]);
        }
        drain();
        __syncthreads();
        if (tid < 64) raise_peers(a, XF_H, 1, gep);
      }
      if (!wait_peers(a, XF_H, 1, gep, ecode(9, s), s_ok)) return;
      // every replica's gradient, summed in rank order
      const auto X = rsrc(a.xbuf[a.rank] + XO_FC2 + (long)par * XMAX * XS_FC2);
      float t[NW + 2];
#pragma unroll
      for (int k = 0; k < NW + 2; ++k) t[k] = 0.f;
      float v[XMAX][NW + 2];  // every peer's gradients in flight before the rank-order sums
#pragma unroll
      for (int r = 0; r < XMAX; ++r) {
        const bool peer = r < a.world && r != a.rank;
        const int o = (int)(r * XS_FC2);
#pragma unroll
        for (int k = 0; k < NW; ++k) v[r][k] = peer ? bld4<SYS>(X, o + (tid + 256 * k) * 4) : gl[k];
        v[r][NW] = peer && tid < HID ? bld4<SYS>(X, o + (NCLS * HID + tid) * 4) : gl[NW];
        v[r][NW + 1] = peer && tid < NCLS ? bld4<SYS>(X, o + (NCLS * HID + HID + tid) * 4) : gl[NW + 1];
      }
#pragma unroll
      for (int r = 0; r < XMAX; ++r)
        if (r < a.world) {
#pragma unroll
          for (int k = 0; k < NW + 2; ++k) t[k] += v[r][k];
        }
#pragma unroll
      for (int k = 0; k < NW + 2; ++k) gl[k] = t[k];
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const int j = tid + 256 * k;
      HW[j] = adadelta(HW[j], gl[k] * hp.gscale, HW1[j], HW2[j], hp);
    }
    if (tid < HID) HB1[tid] = adadelta(HB1[tid], gl[NW] * hp.gscale, HB1[128 + tid], HB1[256 + tid], hp);
    if (tid < NCLS) HB2[tid] = adadelta(HB2[tid], gl[NW + 1] * hp.gscale, HB2[16 + tid], HB2[32 + tid], hp);
    if (i == 0 && tid == 255) {
      float l = 0.f, cc = 0.f;
      for (int b = 0; b < B; ++b) {
        l += ALL[b * PAY + PAY_LOSS];
        cc += ALL[b * PAY + PAY_COR];
      }
      a.out[2 * s] = l * (1.f / B);
      a.out[2 * s + 1] = cc;
    }
    __syncthreads();
    stamp(a, s, 2);
  }
  if (i == 0) {
    for (int j = tid; j < NCLS * HID; j += 256) {
      const long ai = a.off[6] + j;
      a.master[ai] = HW[j];
      a.s1[ai] = HW1[j];
      a.s2[ai] = HW2[j];
      a.shadow[ai] = f2bf_hw(HW[j]);
    }
    if (tid < NCLS) {
      const long ai = a.off[7] + tid;
      a.master[ai] = HB2[tid];
      a.s1[ai] = HB2[16 + tid];
      a.s2[ai] = HB2[32 + tid];
      a.shadow[ai] = f2bf_hw(HB2[tid]);
    }
    if (tid < HID) {
      const long ai = a.off[5] + tid;
      a.master[ai] = HB1[tid];
      a.s1[ai] = HB1[128 + tid];
      a.s2[ai] = HB1[256 + tid];
      a.shadow[ai] = f2bf_hw(HB1[tid]);
    }
  }
}

template <bool DP>
__global__ __launch_bounds__(256, 1) void mnist_persist_k(const Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int s_ok[3];  // [0] a wait's verdict, [1] the multi-wave wait's done word (wait_all), [2] a sweep gave up
  stamp(a, 0, 13);  // (debug stamps: workgroup entry, before the launch prologue)
  if (threadIdx.x == 0) s_ok[0] = s_ok[1] = s_ok[2] = 0;  // (read after the first barrier of either role)
  const OptHP hp = load_hp(a.hp, a.hp_dev);
  const long long cur0 = a.cursor[0];
  const long long xs0 = DP ? a.xstep[0] : 0;
  const unsigned long long eb = *(const unsigned long long*)(a.flags + FL_EPOCH);
  if (blockIdx.x < NPOS) {
    position_wg<DP>(a, smem, s_ok, hp, cur0, a.rng[0], a.rng[1], xs0, eb);
  } else {
    head_wg<DP>(a, smem, s_ok, hp, cur0, xs0, eb);
  }
}

}  // namespace mnistp

// ptrs: master shadow s1 s2 xs ys cursor rng step_dev hp_dev slabA slabB slabC slabD flags err out dbg(0 = none)
//       [xstep xbuf[world] xflag[world]]   (world > 1: the data-parallel instantiation)
//       flags: FL_WORDS + TG_WORDS 32-bit words, zeroed (geom[8] + geom[22]: the tag granules follow the flag rows)
// iv:   off[8] nbatch salt nsteps batch acquire world rank loopback timeout_ms xfence
// fv:   drop_p xscale xshift lr gscale wd rho eps
static int g_persist_reload = 0;
extern "C" void hopsx_mnist_persist_reload_knobs() { g_persist_reload = 1; }
// Args::hand of the last launch (0 before the first): what the knobs came to, for the tests that compare settings.
// One word per process: with several engines or loopback ranks it is whichever launched last (the knobs themselves are
// per process too, so every launch between two reloads carries the same word)
static int g_persist_hand = 0;
extern "C" int hopsx_mnist_persist_hand() { return g_persist_hand; }

extern "C" int hopsx_mnist_persist(const uint64_t* p, int np, const long* iv, int ni, const float* fv, int nf,
                                   hipStream_t st) {
  using namespace mnistp;
  if (np < 18 || ni < 18 || nf < 8) return (int)hipErrorInvalidValue;
  if (iv[11] != B || iv[10] < 1 || iv[8] < 1) return (int)hipErrorInvalidValue;
  const int world = (int)iv[13], rank = (int)iv[14];
  if (world < 1 || world > XMAX || rank < 0 || rank >= world) return (int)hipErrorInvalidValue;
  const bool dp = world > 1;
  if (dp && np < 19 + 2 * world) return (int)hipErrorInvalidValue;
  Args a{};
  a.master = (float*)p[0];
  a.shadow = (bf16_raw*)p[1];
  a.s1 = (float*)p[2];
  a.s2 = (float*)p[3];
  a.xs = (const unsigned char*)p[4];
  a.ys = (const long long*)p[5];
  a.cursor = (long long*)p[6];
  a.rng = (unsigned long long*)p[7];
  a.step_dev = (float*)p[8];
  a.hp_dev = (const float*)p[9];
  a.slabA = (float*)p[10];
  a.slabB = (float*)p[11];
  a.slabC = (float*)p[12];
  a.slabD = (float*)p[13];
  a.flags = (unsigned*)p[14];
  a.err = (unsigned*)p[15];
  a.out = (float*)p[16];
  a.dbg = (unsigned long long*)p[17];
  // the slice owners read whole 128-byte lines of slabC and write whole lines of slabD: both line-aligned
  if (((uint64_t)a.slabC & 127) || ((uint64_t)a.slabD & 127)) return (int)hipErrorInvalidValue;
  for (int k = 0; k < 8; ++k) a.off[k] = iv[k];
  a.nbatch = iv[8];
  a.salt = (unsigned)iv[9];
  a.nsteps = (int)iv[10];
  a.acquire = (int)iv[12];
  a.world = world;
  a.rank = rank;
  a.loopback = (int)iv[15];
  a.xfence = (int)iv[17];
  a.tmo = (long long)iv[16] * 100000ll;  // ms -> 100 MHz ticks
  a.tmo0 = a.tmo;
  // launch knobs (environment), read once and again after hopsx_mnist_persist_reload_knobs (tools/persist_ab.py)
  static int kn_ok = 0, kn_pollw, kn_stagger, kn_a, kn_b, kn_c, kn_d, kn_head1w, kn_memset, kn_coop;
  static int kn_tagged, kn_gate, kn_poll1, kn_prog, kn_fill, kn_fmax;
  static int kn_gate_a, kn_gate_a_tk, kn_head, kn_wlocal;
  static long kn_start_ms;
  if (!kn_ok || g_persist_reload) {
    auto pw = [&](const char* name, long dflt) {
      const long v = hopsx_env_int(name, dflt);
      return (int)(v >= 1 && v <= 4 ? v : 1);
    };
    kn_pollw = pw("HOPSX_PERSIST_POLLW", 1);
    kn_stagger = (int)hopsx_env_int("HOPSX_PERSIST_STAGGER", 12);
    // per hand-off: the slice owners' wait on the 169 conv-gradient partials polls from 4 waves by default
    // (C hop 2.6 -> 1.9 us, 27.6 -> 26.0 us/step: profiles/r5_persist_pollw_ab.txt); the same on the other
    // waits measured slower (more pollers on the flag lines)
    kn_a = pw("HOPSX_PERSIST_POLLW_A", kn_pollw);
    kn_b = pw("HOPSX_PERSIST_POLLW_B", kn_pollw);
    kn_c = pw("HOPSX_PERSIST_POLLW_C", 4);
    kn_d = pw("HOPSX_PERSIST_POLLW_D", kn_pollw);
    kn_head1w = (int)hopsx_env_int("HOPSX_PERSIST_HEAD1W", 1);  // 25.8 -> 25.5 us/step (same profile)
    kn_memset = (int)hopsx_env_int("HOPSX_PERSIST_MEMSET", 0);  // (the round-4 form, for A/B)
    // co-residency: step 0's local hand-offs give up after HOPSX_PERSIST_START_MS (every workgroup starts
    // within microseconds when the grid is resident; anything else means a concurrent kernel holds CUs the
    // grid needs): measured 50 ms to the co-residency error with a kernel holding 128 CUs, instead of the
    // 2 s / 60 s hand-off timeout.  HOPSX_PERSIST_COOP=1 launches cooperatively instead: ROCm then checks
    // the grid against the device's capacity only (what launchable() already does), not against kernels
    // already resident, and costs 0.6 us/step at 32 steps per launch (1.226M -> 1.200M img/s,
    // profiles/r6_persist_dp_sim.txt), so it is off by default
    kn_coop = (int)hopsx_env_int("HOPSX_PERSIST_COOP", 0);
    kn_start_ms = hopsx_env_int("HOPSX_PERSIST_START_MS", 50);
    // the positions read dh from tagged granules instead of payload + drain + flag; HOPSX_PERSIST_TAGGED=0 is
    // the flag form (25.2 -> 23.5 us/step: tools/persist_ab.py, profiles/r7_persist_tagged.txt).  _GATE: heads
    // whose tag opens the B sweep (1, 4, 16, 24, 32 measured: 16 and 24 are 0.2-0.3 us/step faster than 1 and
    // 32 — opened by the first head, every workgroup sweeps through the heads' skew; opened by the last, the
    // sweep starts a poll period late).  _POLL1: the flag polls load the error word with the flags (one round
    // trip per poll: 0.15 us/step)
    kn_tagged = hopsx_env_int("HOPSX_PERSIST_TAGGED", 1) != 0;
    const long gt = hopsx_env_int("HOPSX_PERSIST_GATE", NHEAD / 2);
    kn_gate = (int)(gt >= 1 && gt <= NHEAD ? gt : NHEAD / 2);
    kn_poll1 = hopsx_env_int("HOPSX_PERSIST_POLL1", 1) != 0;
    // progressive fan-in (gather_rows): bit 1 the slice owners' C partials (23.6 -> 23.0 us/step,
    // profiles/r9_persist_progressive.txt); without it C is in the flag form (poll all, barrier, load), the only
    // one HOPSX_PERSIST_POLLW_C still acts on.  Bit 0 was the heads' A rows: measured slower, not in the tree,
    // ignored (so 3, the default, is 2 and 1 is 0)
    kn_prog = (int)(hopsx_env_int("HOPSX_PERSIST_PROG", 3) & 2);
    // waits filled with work that is ready early (position_wg; profiles/r17_persist_fill_waits.txt), one bit per
    // part, default all: 1 the owners' fc1 slice Adadelta inside the progressive C gather (<false>, needs _PROG),
    // 2 the next step's dropout mask drawn in the B wait.  _FILL_MAX caps the chunks (of FCH fc1 updates, NFCH in
    // all) that part 1 runs inside the wait — how many fit depends on timing otherwise; 0 is the old placement
    // through the new path.  No bit and no cap changes a result.  bench.py +4 % with both; 8 updates a chunk and
    // a third part (D's conv2 weights held in registers over the next step's conv1) measured no gain: not in the tree
    kn_fill = (int)(hopsx_env_int("HOPSX_PERSIST_FILL", 3) & 3);
    const long fm = hopsx_env_int("HOPSX_PERSIST_FILL_MAX", NFCH);
    kn_fmax = (int)(fm >= 0 && fm <= NFCH ? fm : NFCH);
    // the heads' A-to-B chain (head_wg; profiles/r18_persist_head_chain.txt).  _GATE_A: the one-line gate in front
    // of the A wait, 0 none, 1 head i on line i % 6, 2 every head on line 0 (one process, 12 alternated reps:
    // 21.77 / 21.49 / 22.30 us/step for 0 / 1 / 2: 1 is the default; 32 pollers on ONE line are worse than none).
    // _GATE_A_US: how long the gate watches before the full wait takes over (0: it gives way after one look).  The
    // default, 20 us, is above the heads' longest A wait in a normal step (stamps, end of the fc2 update -> A ready,
    // max over heads and steps: 10.0 us in one process, 10.7 / 13.0 us at loopback 2 / 8; step 0 from workgroup
    // entry: 15.7 us, where the gate may give way early — it only hands over to the full wait).  _HEAD_CHAIN, one
    // bit per part, default both: 1 the one-wave head's operands in registers from the top of the step (-0.10
    // us/step alone, -0.09 on top of 2), 2 its logits by wave_sum_tree (-0.60); all three parts: 21.77 -> 20.81
    const long ga = hopsx_env_int("HOPSX_PERSIST_GATE_A", 1);
    kn_gate_a = (int)(ga >= 0 && ga <= 2 ? ga : 0);
    const long gus = hopsx_env_int("HOPSX_PERSIST_GATE_A_US", 20);
    kn_gate_a_tk = (int)(gus >= 0 && gus <= 1000000 ? gus * 100 : 2000);  // us -> 100 MHz ticks
    kn_head = (int)(hopsx_env_int("HOPSX_PERSIST_HEAD_CHAIN", 3) & 3);
    // the positions' wave-local staging (position_wg; profiles/r21_persist_wave_local.txt), one bit per part, default
    // all: 1 the forward up to the pooled tile without workgroup barriers, 2 A published per wave, 4 the backward
    // with one barrier and C's part 1 published per wave; 0 is the path of the build before it
    kn_wlocal = (int)(hopsx_env_int("HOPSX_PERSIST_WLOCAL", 7) & 7);
    kn_ok = 1;
    g_persist_reload = 0;
  }
  a.pollw = kn_pollw;
  a.stagger = kn_stagger;
  a.pollw_a = kn_a;
  a.pollw_b = kn_b;
  a.pollw_c = kn_c;
  a.pollw_d = kn_d;
  a.head1w = kn_head1w;
  a.hand = kn_tagged | (kn_poll1 << 1) | (kn_prog << 2) | (kn_gate << 8) | (kn_fill << 16) | (kn_fmax << HAND_FMAX_SHIFT) |
           (kn_gate_a << HAND_GATEA_SHIFT) | (kn_head & 1 ? HAND_HEAD_REGS : 0) | (kn_head & 2 ? HAND_HEAD_TREE : 0) |
           (kn_wlocal & 1 ? HAND_WL_FWD : 0) | (kn_wlocal & 2 ? HAND_WL_A : 0) | (kn_wlocal & 4 ? HAND_WL_BWD : 0);
  g_persist_hand = a.hand;
  a.gate_a_tk = kn_gate_a_tk;
  if (kn_start_ms > 0 && kn_start_ms * 100000ll < a.tmo) a.tmo0 = kn_start_ms * 100000ll;
  a.inv_gb = 1.f / (float)(world * B);
  if (dp) {
    a.xstep = (long long*)p[18];
    for (int r = 0; r < world; ++r) {
      a.xbuf[r] = (unsigned char*)p[19 + r];
      a.xflag[r] = (unsigned*)p[19 + world + r];
      if (!a.xbuf[r] || !a.xflag[r] || ((uint64_t)a.xbuf[r] & 15)) return (int)hipErrorInvalidValue;
    }
  }
  a.drop_p = fv[0];
  a.xscale = fv[1];
  a.xshift = fv[2];
  a.hp = OptHP{fv[3], fv[4], fv[5], fv[6], fv[7], 0.f, 0.f, 0.f};
  static bool attr[2] = {false, false};
  const void* fn = dp ? (const void*)mnist_persist_k<true> : (const void*)mnist_persist_k<false>;
  if (!attr[dp]) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    if (e != hipSuccess) return (int)e;
    attr[dp] = true;
  }
  if (kn_memset) {  // (the round-4 form, for A/B: zeroed flags each launch)
    const hipError_t e = hipMemsetAsync(a.flags, 0, FL_WORDS * sizeof(unsigned), st);
    if (e != hipSuccess) return (int)e;
  }
  if (kn_coop) {
    // cooperative launch: refused at once (hipErrorCooperativeLaunchTooLarge) when the device cannot hold
    // all GRID workgroups together, instead of workgroups spinning on hand-offs that cannot come
    void* kargs[] = {(void*)&a};
    const hipError_t e = hipLaunchCooperativeKernel(fn, dim3(GRID), dim3(256), kargs, LDS_BYTES, st);
    if (e != hipSuccess) {
      (void)hipGetLastError();  // clear the sticky launch error; the caller raises on the return code
      return (int)e;
    }
    return (int)hipSuccess;
  }
  if (dp)
    hipLaunchKernelGGL(mnist_persist_k<true>, dim3(GRID), dim3(256), LDS_BYTES, st, a);
  else
    hipLaunchKernelGGL(mnist_persist_k<false>, dim3(GRID), dim3(256), LDS_BYTES, st, a);
  return (int)hipGetLastError();
}

// Workgroups of the persistent kernel one CU can hold at once (registers, LDS, wave slots): the
// launch hands data between workgroups, so all GRID of them must be co-resident — the host requires
// this >= 1 and CUs >= GRID before it picks the persistent engine (runtime/persist.py launchable()).
extern "C" int hopsx_mnist_persist_occupancy(int dp) {
  using namespace mnistp;
  const void* fn = dp ? (const void*)mnist_persist_k<true> : (const void*)mnist_persist_k<false>;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess) return -1;
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, 256, LDS_BYTES) != hipSuccess) return -1;
  return n;
}

// geometry for the host wrapper (buffer sizes) and the tests
extern "C" void hopsx_mnist_persist_geom(long* g) {
  using namespace mnistp;
  g[0] = B;
  g[1] = NPOS;
  g[2] = NHEAD;
  g[3] = GRID;
  g[4] = NCONV;
  g[5] = NSLICE;
  g[6] = SLICE;
  g[7] = PAY;
  g[8] = FL_WORDS;
  g[9] = LDS_BYTES;
  g[10] = D_BYTES;
  g[11] = X_BYTES;
  g[12] = XF_WORDS;
  g[13] = XMAX;
  // exchange-buffer layout (runtime/persist_sim.py): region offset, per-slot bytes, for the pooled
  // fragments, dh^T fragments, head gradients and conv slice sums ([2 parities][XMAX slots] each)
  g[14] = XO_POOL;
  g[15] = XS_POOL;
  g[16] = XO_DHT;
  g[17] = XS_DHT;
  g[18] = XO_FC2;
  g[19] = XS_FC2;
  g[20] = XO_CONV;
  g[21] = XS_CONV;
  g[22] = TG_WORDS;  // tag granules of hand-off B behind the flag rows (32-bit words)
  g[23] = NFCH;      // chunks of the fc1 slice update (the range of HOPSX_PERSIST_FILL_MAX)
}

// Probe of common.h wave_sum_tree against wave_sum (tests/test_wave_sum_tree_gpu.py): one wave per row of 64 values,
// every lane's result of both, out_ref / out_tree [rows][64]
__global__ __launch_bounds__(64) void wave_sum_probe_k(const float* x, float* out_ref, float* out_tree) {
  const long e = (long)blockIdx.x * 64 + threadIdx.x;
  const float v = x[e];
  out_ref[e] = wave_sum(v);
  out_tree[e] = wave_sum_tree(v);
}
extern "C" int hopsx_wave_sum_probe(const float* x, long rows, float* out_ref, float* out_tree, hipStream_t st) {
  if (rows < 1 || rows > 65535 || !x || !out_ref || !out_tree) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(wave_sum_probe_k, dim3((unsigned)rows), dim3(64), 0, st, x, out_ref, out_tree);
  return (int)hipGetLastError();
}
