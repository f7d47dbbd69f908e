// The gfx950 (CDNA4) device primitives every MFMA kernel file shares, each defined once: buffer
// descriptor, wait counts and barriers, the 16-byte-per-lane LDS-DMA in its two forms, the
// inline-asm MFMAs, the accumulator pins and the transposed fragment read.  Variants that differ
// on purpose sit next to their relatives under their own names.
#pragma once
#include <utility>
#include "common.h"

namespace cxg {

typedef __amdgpu_buffer_rsrc_t rsrc_t;
typedef __attribute__((address_space(3))) void lds_void;

// Buffer loads: 32-bit byte offsets against a wave-uniform resource descriptor; an offset past
// num_records returns zeros, so padding / ragged edges need no branches.
__device__ __forceinline__ rsrc_t make_rsrc(const void *p, uint32_t nbytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), (short)0, static_cast<int>(nbytes), 0x00020000);
}

// ------------------------------------------------------------------- wait counts and barriers
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_lgkm() {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ void block_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// Lanes of one wave hand data to each other through LDS (stage, then read back in another
// layout): every LDS operation the wave has issued completes (lgkmcnt(0)), then a wave barrier
// keeps hipcc from moving LDS accesses across the hand-over.  The wait-count form; the fence form
// of the 8-wave GEMM epilogues is wave_lds_handoff<ON> in gemm_glds_common.h.
__device__ __forceinline__ void wave_lds_wait_handoff() {
  wait_lgkm<0>();
  __builtin_amdgcn_wave_barrier();
}

template <typename F, int... I>
__device__ __forceinline__ void static_for_impl(F &&f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
// f(std::integral_constant<int, i>) for i = 0..N-1, fully unrolled with constant indices
template <int N, typename F>
__device__ __forceinline__ void static_for(F &&f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// ------------------------------------------------------------------------------- LDS-DMA
// One 1-KiB LDS-DMA (16 bytes per lane) as inline asm.  hipcc cannot tell the LDS bytes the DMA
// writes (the next stage's / patch's) from the ones the ds_reads of the current stage touch, and
// for the builtin form it inserts a vmcnt(0) before the first ds_read after the DMAs: every stage
// then waited for all of the next stage's HBM loads at its first K-step instead of letting them
// land under its MFMAs (144 of them per patch in conv_wgrad_halo).  As asm, hipcc neither waits
// for the DMA before the current stage's ds_reads nor reorders LDS reads across it; completion is
// counted by hand (wait_vmcnt + barrier at the end of each stage / patch).  M0 is saved and
// restored inside the statement (compiler-reserved).
__device__ __forceinline__ void dma16(rsrc_t r, uint32_t lds_addr, uint32_t voff) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(r), "s"(lds_addr) : "memory");
}

// The same DMA through the builtin, with a descriptor built from (base, records).  A free
// function on purpose: with the builtin called directly inside the kernel's lambdas, hipcc's host
// pass silently dropped the kernel's launch stub (undefined __device_stub__ at load time).
__device__ __forceinline__ void lds_dma16(const char *p, uint32_t n, char *dst, uint32_t voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(make_rsrc(p, n), (lds_void *)dst, 16, voff, 0, 0, 0);
}

// ---------------------------------------------------------------------------------- MFMA
// 16x16x32 bf16 MFMA as inline asm, the accumulator pinned in its AGPRs ("+a"): with the builtin,
// hipcc kept the loop-carried tile in VGPRs and copied all of it into AGPRs and back every stage
// (2 x 96 v_accvgpr moves per stage in conv_direct), or rotated the accumulators through other
// registers.  AGPR = false: accumulators beyond the 256-register AGPR file live in VGPRs (gfx950
// MFMAs take either).  Hazards hipcc does not pad for inline asm: the A/B operands come only from
// ds_read (waited with lgkmcnt; benchmarks/asm_audit.py checks that no VALU writes them in the
// loop); the reads of the accumulators after the loop are padded with s_nop by the callers.
template <bool AGPR = true>
__device__ __forceinline__ void mfma16(f32x4 &acc, const bf16x8 &a, const bf16x8 &b) {
  if constexpr (AGPR) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
  else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
// acc = a b: zero C operand, the accumulator only written ("=a")
__device__ __forceinline__ void mfma_z(f32x4 &acc, const bf16x8 &a, const bf16x8 &b) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=a"(acc) : "v"(a), "v"(b));
}
// bias-gradient MFMA: its B operand (the ones fragment) lives in VGPRs that hipcc may have just
// (re)written with a VALU move; "s_nop 1" covers the VALU-write -> MFMA-operand wait states hipcc
// does not insert for inline asm
__device__ __forceinline__ void mfma_db(f32x4 &acc, const bf16x8 &a, const bf16x8 &b) {
  asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
// 32x32x16 (f32x16 accumulator in AGPRs)
__device__ __forceinline__ void mfma32(f32x16 &acc, const bf16x8 &a, const bf16x8 &b) {
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}

// An empty volatile asm that "rewrites" an accumulator: register code reading or writing it
// cannot move across it, and it keeps its order with the other volatile asm.
template <bool AGPR>
__device__ __forceinline__ void pin(f32x4 &acc) {
  if constexpr (AGPR) asm volatile("" : "+a"(acc));
  else asm volatile("" : "+v"(acc));
}
template <int MR, int NR>
__device__ __forceinline__ void pin_acc(f32x4 (&acc)[MR][NR]) {
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int n = 0; n < NR; ++n) pin<true>(acc[m][n]);
}

// two transposed 8-byte reads (k-rows k and k + 4 of a group of 8: 8 g4 + q and 8 g4 + 4 + q)
// -> one 16x16x32 operand fragment
__device__ __forceinline__ bf16x8 frag_tr(const char *p0, const char *p1) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(p0));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(p1));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}

// floor(a / b) for b > 0
constexpr int fdiv_floor(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

}  // namespace cxg
