// What the attention kernel files share (attn_kernels.hip, kvattn_kernels.hip): the swizzled
// [64][D] bf16 LDS tile, its LDS-DMA staging from strided rows, the row-major and transposed MFMA
// operand fragments, and the small register helpers around the compiler-builtin MFMA; and, in
// namespace row64, the [rows][32] tile of wattn_kernels.hip and nattn_kernels.hip with the swizzle
// a 64-byte row needs (wattn_kernels.hip's header derives it).  See
// attn_kernels.hip's header for why the products are computed transposed and why the MFMAs are the
// builtin and not gfx950_prims.h's asm forms.
#pragma once
#include "gfx950_prims.h"

namespace cxg {
namespace attn {

constexpr uint32_t OOB = 0x80000000u;  // >= num_records: the DMA writes zeros
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;  // (sc2; lse = lse2 ln2)

// byte address of 16-byte unit lc of row r in a [64][D] bf16 tile
template <int D>
__device__ __forceinline__ int tile_addr(int r, int lc) {
  constexpr int CH = D / 8;
  return r * (D * 2) + ((lc ^ (r & (CH - 1))) << 4);
}

// Stage rows row0 .. row0 + 63 of two strided matrices (descriptors ra / rb, row strides sa / sb
// bytes, D columns each) into the tiles at lds and lds + 64 D 2.  One DMA covers 1024 / (2 D) rows;
// wave w issues DMAs w, w + 4, ...; rows >= T get zeros.
template <int D>
__device__ __forceinline__ void stage2(rsrc_t ra, uint32_t sa, rsrc_t rb, uint32_t sb, uint32_t lds, int row0,
                                       int T, int wave, int lane) {
  constexpr int CH = D / 8, RPD = 64 / CH, ND = 64 / RPD, TILE = 64 * D * 2;
  const int pc = lane & (CH - 1), rl = lane / CH;
#pragma unroll
  for (int j = 0; j < 2 * ND / 4; ++j) {
    const bool first = j < ND / 4;
    const int qq = wave + 4 * j - (first ? 0 : ND);
    const int r = qq * RPD + rl;
    const int lc = pc ^ (r & (CH - 1));
    uint32_t off = row0 + r < T ? static_cast<uint32_t>(row0 + r) * (first ? sa : sb) + lc * 16u : OOB;
    asm volatile("" : "+v"(off));  // keep the select: no per-lane branch around the DMA
    dma16(first ? ra : rb, lds + static_cast<uint32_t>((first ? 0 : TILE) + qq * 1024), off);
  }
}

// row-major operand fragment: row r (the lane's), columns 32 ks + 8 g ..
template <int D>
__device__ __forceinline__ bf16x8 row_frag(const char *tile, int r, int ks, int g) {
  return *reinterpret_cast<const bf16x8 *>(tile + tile_addr<D>(r, 4 * ks + g));
}

// transposed operand fragment: lane (i, g) gets column 16 dt + i of rows rb + 4 g + j (slots 0..3)
// and rb + 16 + 4 g + j (slots 4..7) -- the order in which a lane holds two 16 x 16 result tiles
template <int D>
__device__ __forceinline__ bf16x8 tr_frag(const char *tile, int rb, int dt, int i, int g) {
  const int r = rb + 4 * g + (i >> 2);
  const char *p = tile + tile_addr<D>(r, 2 * dt + ((i & 3) >> 1)) + (i & 1) * 8;
  return frag_tr(p, p + 16 * D * 2);  // (row r + 16 has row r's swizzle)
}

__device__ __forceinline__ f32x4 mma(const bf16x8 &a, const bf16x8 &b, const f32x4 &c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// a b rounded to fp32 on its own: the empty asm keeps hipcc from contracting it into the following
// subtraction (an fma would subtract from the unrounded product, and the backward's s - lse2 must
// reproduce the forward's bits: one dominant key then gives P = 1 and dS = 0 exactly)
__device__ __forceinline__ float mul_rn(float a, float b) {
  float x = a * b;
  asm("" : "+v"(x));
  return x;
}

__device__ __forceinline__ bf16x8 pack_frag(const f32x4 &lo, const f32x4 &hi) {
  const uint4 v = make_uint4(pack2(lo[0], lo[1]), pack2(lo[2], lo[3]), pack2(hi[0], hi[1]), pack2(hi[2], hi[3]));
  return __builtin_bit_cast(bf16x8, v);
}

// the lane's 8 columns 32 ks + 8 g .. of a global row; zeros when !ok
template <int KS>
__device__ __forceinline__ void load_row(const bf16_t *row, bool ok, int g, bf16x8 (&f)[KS]) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (ok) v = *reinterpret_cast<const uint4 *>(row + 32 * ks + 8 * g);
    f[ks] = __builtin_bit_cast(bf16x8, v);
  }
}

// 4 columns 16 dt + 4 g .. of a row for every dt, scaled
template <int DT>
__device__ __forceinline__ void store_row(bf16_t *row, int g, const f32x4 (&acc)[DT], float f) {
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
    *reinterpret_cast<uint2 *>(row + 16 * dt + 4 * g) =
        make_uint2(pack2(acc[dt][0] * f, acc[dt][1] * f), pack2(acc[dt][2] * f, acc[dt][3] * f));
}

__device__ __forceinline__ uint32_t lds_base(const char *smem) {
  return __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_void *)smem)));
}

// The [rows][32] bf16 tile with 64-byte rows.  Unit lc of row r lives at physical unit lc ^ swz(r),
// swz(r) = bit 2 of r as bit 1, bit 3 of r as bit 0; the argument needs 16 (row_frag) or 8 (tr_frag)
// consecutive rows, not an aligned first row.
namespace row64 {

__device__ __forceinline__ int swz(int r) { return ((r >> 1) & 2) | ((r >> 3) & 1); }

// byte address of 16-byte unit lc of row r
__device__ __forceinline__ int tile_addr(int r, int lc) { return r * 64 + ((lc ^ swz(r)) << 4); }

// row-major operand fragment: row r, columns 8 g ..
__device__ __forceinline__ bf16x8 row_frag(const char *tile, int r, int g) {
  return *reinterpret_cast<const bf16x8 *>(tile + tile_addr(r, g));
}

// transposed operand fragment: lane (i, g) gets column 16 dt + i of rows rb + 4 g + j (slots 0..3)
// and rb + 16 + 4 g + j (slots 4..7) -- the order in which a lane holds two 16 x 16 result tiles
__device__ __forceinline__ bf16x8 tr_frag(const char *tile, int rb, int dt, int i, int g) {
  const int r = rb + 4 * g + (i >> 2);
  const char *p = tile + tile_addr(r, 2 * dt + ((i & 3) >> 1)) + (i & 1) * 8;
  return frag_tr(p, p + 16 * 64);  // (row r + 16 has row r's swizzle)
}

}  // namespace row64

}  // namespace attn
}  // namespace cxg
