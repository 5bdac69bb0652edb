// hopsx: the device vocabulary of the whole-step kernels (mnist_persist.hip, mnist_eval.hip, taxi_step.hip,
// taxi_eval.hip), defined once.  Each of those files pulls it in with `using namespace wgp;` inside its own
// namespace.  Only definitions that mention no kernel's Args live here; waits, stamps and optimizer
// one-liners stay with their kernels.
#pragma once
#include "common.h"

namespace wgp {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v2i __attribute__((ext_vector_type(2)));
typedef unsigned __attribute__((address_space(1))) gu32;
typedef unsigned long long __attribute__((address_space(1))) gu64;
typedef __attribute__((address_space(3))) bf16x4* lds4_t;

// fp32 -> bf16 round-to-nearest-even by the gfx950 conversion instruction (v_cvt_pk_bf16_f32):
// the same bits as common.h's f2bf for every finite value, one instruction instead of five
__device__ __forceinline__ bf16_raw f2bf_hw(float f) { return __builtin_bit_cast(bf16_raw, (__bf16)f); }
__device__ __forceinline__ float b2f(short v) { return __uint_as_float(((uint32_t)(uint16_t)v) << 16); }

// ---- LDS fragment reads ----
__device__ __forceinline__ bf16x8 lds8(const bf16_raw* p) { return *(const bf16x8*)p; }
// transposed fragment read (ds_read_b64_tr_b16): within each group of 16 lanes, lane i addresses row i >> 2,
// 4 consecutive columns 4 * (i & 3)..; the result holds column i's 4 row values.  EXEC must be full: never
// call under a lane-dependent branch.
__device__ __forceinline__ bf16x4 lds_tr4(const bf16_raw* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4_t)p);
}
// the pair for a 16x16x32 operand: this lane addresses row (k) 8*fq + tq (p1) and 8*fq + tq + 4 (p2),
// 4 consecutive columns 4*tp..; the result holds column (lane & 15)'s 8 k values
__device__ __forceinline__ bf16x8 lds_tr(const bf16_raw* p1, const bf16_raw* p2) {
  const bf16x4 v1 = lds_tr4(p1);
  const bf16x4 v2 = lds_tr4(p2);
  return (bf16x8){v1[0], v1[1], v1[2], v1[3], v2[0], v2[1], v2[2], v2[3]};
}

// ---- MFMA ----
__device__ __forceinline__ f32x4 mma32(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mma16(bf16x4 a, bf16x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}
// The held forms, for a kernel that keeps MFMA operands in registers across the MFMA (taxi_eval.hip).
// The MFMA reads its A / B registers over its first cycles, and nothing interlocks a VALU write to them in
// that window: with the activations living in registers, hipcc reused the last A register for an address
// computation in the very next instruction after a 16x16x32 (`v_mfma ... v[118:121] ...; v_add_u32 v121, ...`)
// and the product came out wrong.  The pad keeps A and B alive (and every later write to their registers
// behind it) for 4 wait states after the issue; it is inside the string, where no pass can separate them.
__device__ __forceinline__ f32x4 mma32_held(bf16x8 a, bf16x8 b, f32x4 c) {
  f32x4 r = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  asm volatile("s_nop 3" : "+v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ f32x4 mma16_held(bf16x4 a, bf16x4 b, f32x4 c) {
  f32x4 r = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
  asm volatile("s_nop 3" : "+v"(r) : "v"(a), "v"(b));
  return r;
}

// ---- buffer stores / loads of the hand-off payloads ----
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, 0x7fffffff, 0x00020000);
}
// cache policy (the builtins' aux operand).  SC1: write-through store / L1-bypassing load, the hand-off
// path between workgroups of one device.  SYS (sc0 sc1): system scope, the cross-rank exchange path on the
// uncached exchange buffers.
constexpr int SC1 = 16, SYS = 17;
template <int POL>
__device__ __forceinline__ void bst16(__amdgpu_buffer_rsrc_t r, int byte_off, f32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i, v), r, byte_off, 0, POL);
}
// (two 32-bit words, int or float each)
template <int POL, class X, class Y>
__device__ __forceinline__ void bst8(__amdgpu_buffer_rsrc_t r, int byte_off, X x, Y y) {
  __builtin_amdgcn_raw_buffer_store_b64((v2i){__builtin_bit_cast(int, x), __builtin_bit_cast(int, y)}, r, byte_off, 0, POL);
}
template <int POL>
__device__ __forceinline__ void bst4(__amdgpu_buffer_rsrc_t r, int byte_off, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, byte_off, 0, POL);
}
template <int POL>
__device__ __forceinline__ f32x4 bld16(__amdgpu_buffer_rsrc_t r, int byte_off) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, POL));
}
template <int POL>
__device__ __forceinline__ v2i bld8(__amdgpu_buffer_rsrc_t r, int byte_off) {
  return __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, 0, POL);
}
template <int POL>
__device__ __forceinline__ float bld4(__amdgpu_buffer_rsrc_t r, int byte_off) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, POL));
}
// every vector memory operation of this wave has completed (a storing wave drains before its flag goes up)
__device__ __forceinline__ void drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ---- flag words: relaxed, agent scope (one device) and system scope (cross-rank, x) ----
__device__ __forceinline__ void flag_store(unsigned* f, unsigned v) {
  __hip_atomic_store((gu32*)f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned flag_load(const unsigned* f) {
  return __hip_atomic_load((gu32*)f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void xflag_store(unsigned* f, unsigned v) {
  __hip_atomic_store((gu32*)f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ unsigned xflag_load(const unsigned* f) {
  return __hip_atomic_load((gu32*)f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Workgroup barrier that waits only for LDS traffic: global loads stay in flight across it (a
// __syncthreads() would drain them at every phase)
__device__ __forceinline__ void bar() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

}  // namespace wgp
