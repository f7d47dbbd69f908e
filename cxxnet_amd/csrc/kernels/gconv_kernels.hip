// Narrow-group 3 x 3 convolution (ngroup >= 4 groups of 4, 8, 16 or 32 channels: the grouped conv of
// ResNeXt / aggregated-transform nets) on block-diagonal MFMAs.  Such a layer has 9 cg MACs per
// output and reads every input once: it is bound by the bytes it moves, a GEMM per group has cg
// rows, and a stencil per channel has a cg-wide reduction.  Here several groups share one
// v_mfma_f32_16x16x32_bf16 and the arithmetic rides along for free.
//
//   cxn_gconv_fwd         y  = [relu](conv(x, w) + bias)
//   cxn_gconv_bwd_data    dx = conv_transpose(dy, w) [masked by relu'(z), dx = relu(z) on entry]
//   cxn_gconv_bwd_weight  dw += sum over pixels of dy (x) x                      (two launches)
//
// Served: groups >= 4, C == Cout, C % 16 == 0, cg = C / groups in {4, 8, 16, 32}, KH == KW == 3,
// pad_y == pad_x == 1, stride in {1, 2}; everything else returns -1.  Activations are NHWC bf16
// with an explicit pixel stride in elements (a node may be a channel slice of a wider buffer),
// weights [Cout][3][3][cg] bf16, accumulation fp32, one rounding.
//
// Channel blocks and units.  The channels are cut into blocks of CB = 16 (cg <= 16) or 32
// (cg = 32) whole groups; a unit is 16 consecutive channels (a 16-block, or half a 32-block).  One
// MFMA gives 16 channels of one unit x 16 pixels.  Its K = 32 is two taps x the 16 channels of the
// block (CB = 16: ten half-steps for nine taps, five K-steps) or one tap x the 32 channels (CB =
// 32: nine K-steps).  The weight operand of a K-step is the block-diagonal matrix of the block's
// groups.  It is built in LDS from w itself -- zero fill, then the cg-wide pieces -- once per
// block of threads; each wave keeps the 5 / 9 fragments of its unit in registers for its whole walk.
// The data gradient places the same pieces transposed and in its own tap order: there is no dense
// and no flipped copy of the weights in global memory.
//
// Patches.  A block of threads (4 waves) owns a slice of NU = 4, 2 or 1 units (128 contiguous
// bytes per pixel where C % 64 == 0) and walks patches of one image: R x 16 output pixels
// (forward, stride-1 data gradient, weight gradient; R = 8 at stride 1, 4 at stride 2).  The input
// halo of the patch -- ((R - 1) S + 3) x (15 S + 3) pixels -- is staged once by LDS-DMA, 16 bytes
// per lane; a pixel outside the image is a load past the buffer's records, which writes zeros:
// borders cost no branch and no padded copy.  A halo pixel is a slot of 32 NU bytes, rows are
// P = 24 or 40 slots (P % 8 == 0), and the 16-byte chunk c of slot s holds logical chunk
// c ^ (s % (2 NU)): the key follows the column, so a tap is a constant byte offset per lane and
// the 16 pixels of a fragment read distinct bank groups (conv_halo.hip's scheme).  At stride 2 a
// fragment reads every second slot.
//
// Stride-2 data gradient.  The dy halo is 9 x 17 pixels for a 16 x 32 patch of dx.  A dx pixel
// belongs to one of four classes (row parity x column parity) with 1, 2, 2 and 4 taps; 16 pixels
// of one class and one row are one fragment, and the ten half-steps are laid out class by class
// (S2_ORDER), so the classes take 1, 1, 1 and 2 K-steps at CB = 16 and 1, 2, 2, 4 at CB = 32.
//
// Weight gradient.  Per (output unit, input unit) of a block and per tap, dy^T x over the pixels:
// K = 32 pixels = two patch rows.  Both operands are pixel-major, so both are read transposed
// (frag_tr).  9 accumulators per unit pair; of each 16 x 16 result only the elements whose two
// channels share a group are kept.  The patches are cut into P slabs (mirrored by
// ops.gemm.gconv_wgrad_partials); a block reduces one slab for its slice into the fp32 workspace,
// and a second launch merges the slabs in a fixed order onto dw.  No atomics: the same bits on
// every run, in every mode.
#include "gemm_glds_common.h"

using namespace cxg;

namespace {

constexpr int NT = 256;
constexpr int PMAX = 512;       // weight gradient: slabs to aim for (over all slices)
constexpr int BLOCKS = 1024;    // forward / data gradient: blocks to aim for

enum { FWD = 0, DGRAD1 = 1, DGRAD2 = 2 };

// Tile geometry.  ROWS x 16 fragments of 16 pixels; the halo is HR x HC slots in rows of P; the
// patch covers PH x PW pixels of the tensor the items walk; OFF: the halo's origin relative to the
// patch's first source pixel.
template <int S, int MODE>
struct Tile {
  static constexpr int ROWS = MODE == DGRAD2 ? 8 : (S == 1 ? 8 : 4);
  static constexpr int ST = MODE == DGRAD2 ? 1 : S;    // slots between neighbouring pixels of a fragment
  static constexpr int HR = MODE == DGRAD2 ? ROWS + 1 : (ROWS - 1) * S + 3;
  static constexpr int HC = MODE == DGRAD2 ? 17 : 15 * S + 3;
  static constexpr int P = (HC + 7) / 8 * 8;
  static constexpr int OFF = MODE == DGRAD2 ? 0 : -1;
  static constexpr int PH = MODE == DGRAD2 ? 2 * ROWS : ROWS;
  static constexpr int PW = MODE == DGRAD2 ? 32 : 16;
  static constexpr int HALO = (HR * P * 128 + 1023) / 1024 * 1024;  // bytes at NU = 4
};

// The stride-2 data gradient's tap order, class by class: (1,1) | (1,0) (1,2) | (0,1) (2,1) |
// (0,0) (0,2) (2,0) (2,2), as tap indices kh * 3 + kw.
constexpr uint64_t S2_ORDER = 0x862071534ull;  // nibble i: the i-th tap
constexpr int s2_tap(int i) { return i < 9 ? static_cast<int>((S2_ORDER >> (4 * i)) & 15u) : -1; }
static_assert(s2_tap(0) == 4 && s2_tap(1) == 3 && s2_tap(2) == 5 && s2_tap(3) == 1 && s2_tap(4) == 7 && s2_tap(5) == 0 &&
              s2_tap(6) == 2 && s2_tap(7) == 6 && s2_tap(8) == 8, "tap order");
// tap of K-slot s (a half-step at CB = 16, where slot 1 is the empty half of class 0; a K-step at
// CB = 32); -1: none
constexpr int tap_of_slot(int cb, int mode, int s) {
  if (mode == FWD) return s < 9 ? s : -1;
  if (mode == DGRAD1) return s < 9 ? 8 - s : -1;
  if (cb == 32) return s2_tap(s);
  return s == 0 ? 4 : (s == 1 ? -1 : s2_tap(s - 1));
}
// the inverse as packed nibbles (nibble t: the slot of tap t), checked against tap_of_slot
constexpr uint64_t slot_nibbles(int cb, int mode) {
  uint64_t v = 0;
  for (int s = 0; s < (cb == 16 ? 10 : 9); ++s) {
    const int t = tap_of_slot(cb, mode, s);
    if (t >= 0) v |= static_cast<uint64_t>(s) << (4 * t);
  }
  return v;
}
static_assert(slot_nibbles(16, DGRAD2) == 0x958302746ull && slot_nibbles(32, DGRAD2) == 0x847201635ull, "tap order");
// first K-step and K-step count of parity class cls = 2 rp + cp
constexpr int cls_first(int cb, int cls) { return cb == 16 ? cls : (cls == 0 ? 0 : (cls == 1 ? 1 : (cls == 2 ? 3 : 5))); }
constexpr int cls_count(int cb, int cls) { return cb == 16 ? (cls == 3 ? 2 : 1) : (cls == 0 ? 1 : (cls == 3 ? 4 : 2)); }

struct GArgs {
  int N, Hs, Ws;      // the staged tensor (forward / weight gradient: x; data gradient: dy)
  int Hd, Wd;         // the tensor the items walk (forward: y; data gradient: dx; weight gradient: dy)
  int C, cg, lg, NU;  // lg = log2 cg; NU units (of 16 channels) per slice
  long ps_s, ps_d;    // pixel strides in elements
  uint32_t s_bytes, d_bytes;  // byte extents of the two views, < 2^31
  uint32_t items, tw, thw;    // patches, patches per row, patches per image
  FastDiv dtw, dthw;
};

__device__ __forceinline__ void item_of(const GArgs &a, uint32_t it, int &n, int &ph, int &pw) {
  const uint32_t nn = fdiv(it, a.dthw);
  const uint32_t rem = it - nn * a.thw;
  const uint32_t hh = fdiv(rem, a.dtw);
  n = static_cast<int>(nn);
  ph = static_cast<int>(hh);
  pw = static_cast<int>(rem - hh * a.tw);
}

// byte address of logical 16-byte chunk lc of slot `slot`; sb bytes per slot, ncm = chunks per slot - 1
__device__ __forceinline__ int slot_addr(int slot, int lc, int sb, int ncm) {
  return slot * sb + ((lc ^ (slot & ncm)) << 4);
}

// Stage HR x HC pixels (rows of P slots) of image n from source pixel (oy, ox) on, channels of the
// slice at `base`: 1-KiB LDS-DMA groups, group q = slots q (32 / NU) ..., lane -> slot q (32 / NU) +
// lane / NC, physical chunk lane % NC.  Slots outside the image or past the halo get zeros.
template <int HR, int HC, int P>
__device__ __forceinline__ void stage(char *dst, const char *base, uint32_t nbytes, int n, int oy, int ox, int H,
                                      int W, long ps, int NU, int wave, int lane) {
  const int nc = 2 * NU, spg = 32 / NU;
  const int ng = (HR * P * NU * 32 + 1023) / 1024;
  const int pc = lane & (nc - 1), sl = lane / nc;
  for (int q = wave; q < ng; q += 4) {
    const int slot = q * spg + sl;
    const int hr = slot / P, hc = slot - hr * P;
    const int gh = oy + hr, gw = ox + hc;
    const bool ok = hr < HR && hc < HC && static_cast<unsigned>(gh) < static_cast<unsigned>(H) &&
                    static_cast<unsigned>(gw) < static_cast<unsigned>(W);
    const int lc = pc ^ (slot & (nc - 1));
    uint32_t off = ok ? static_cast<uint32_t>((n * H + gh) * W + gw) * static_cast<uint32_t>(ps) * 2u + lc * 16u : OOB;
    asm volatile("" : "+v"(off));  // keep the select: no per-lane branch around the DMA
    lds_dma16(base, nbytes, dst + q * 1024, off);
  }
}

// The block-diagonal weight operand of the slice at channel c0 in LDS: unit u, K-step ks is a
// [16 rows][32 k] bf16 matrix at (u KS + ks) 1024.  Forward: row = output channel, k = input
// channel of the block (+ 16 for the second tap of a pair); data gradient: the transpose.
template <int CB, int MODE>
__device__ __forceinline__ void build_w(char *wl, const bf16_t *__restrict__ w, int c0, int NU, int cg, int lg) {
  constexpr int KS = CB == 16 ? 5 : 9;
  constexpr uint64_t NIB = slot_nibbles(CB, MODE);
  const int tid = threadIdx.x;
  for (int e = tid; e < NU * KS * 64; e += NT) reinterpret_cast<uint4 *>(wl)[e] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  const int npiece = NU * 16 * 9 * (cg >> 2);  // runs of 4 input channels
  for (int e = tid; e < npiece; e += NT) {
    const int q = e & ((cg >> 2) - 1);
    const int r = e >> (lg - 2);
    const int co_s = r / 9, tap = r - co_s * 9;
    const uint2 v = *reinterpret_cast<const uint2 *>(w + (static_cast<size_t>(c0 + co_s) * 9 + tap) * cg + 4 * q);
    const int blk = co_s / CB, co_b = co_s % CB;
    const int ci_b = ((co_b >> lg) << lg) + 4 * q;  // first of the run's input channels within the block
    const int slot = static_cast<int>((NIB >> (4 * tap)) & 15u);
    const int ks = CB == 16 ? slot >> 1 : slot;
    const int kb = CB == 16 ? (slot & 1) * 16 : 0;
    if constexpr (MODE == FWD) {
      const int unit = CB == 16 ? blk : 2 * blk + (co_b >> 4);
      *reinterpret_cast<uint2 *>(wl + (unit * KS + ks) * 1024 + (co_b & 15) * 64 + (kb + ci_b) * 2) = v;
    } else {
      const uint32_t h[4] = {v.x & 0xffffu, v.x >> 16, v.y & 0xffffu, v.y >> 16};
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int row = ci_b + m;
        const int unit = CB == 16 ? blk : 2 * blk + (row >> 4);
        *reinterpret_cast<bf16_t *>(wl + (unit * KS + ks) * 1024 + (row & 15) * 64 + (kb + co_b) * 2) =
            static_cast<bf16_t>(h[m]);
      }
    }
  }
  __syncthreads();
}

// ------------------------------------------------------- forward and data gradient (one product)
// flag: relu (forward) / mask_relu (data gradient)
template <int CB, int S, int MODE>
__global__ __launch_bounds__(NT) void gconv_mm(const bf16_t *__restrict__ src, const bf16_t *__restrict__ w,
                                               const float *__restrict__ bias, bf16_t *dst, const GArgs a, int flag) {
  using T = Tile<S, MODE>;
  constexpr int KS = CB == 16 ? 5 : 9, P = T::P, ST = T::ST;
  __shared__ __attribute__((aligned(1024))) char smem[T::HALO + 4 * KS * 1024];
  char *halo = smem, *wl = smem + T::HALO;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l16 = lane & 15, g4 = lane >> 4;
  const int NU = a.NU, sb = NU * 32, ncm = 2 * NU - 1;
  const int c0 = blockIdx.y * NU * 16;
  build_w<CB, MODE>(wl, w, c0, NU, a.cg, a.lg);

  const int unit = wave & (NU - 1);     // this wave's 16 channels of the slice
  const int fg = wave / NU, FG = 4 / NU;  // and its share of the patch's fragment rows
  bf16x8 af[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    af[ks] = *reinterpret_cast<const bf16x8 *>(wl + (unit * KS + ks) * 1024 + l16 * 64 + g4 * 16);
  // the lane's 8 k-values of a K-step: CB = 16: tap half g4 / 2, channels 8 (g4 % 2) .. of the block;
  // CB = 32: channels 8 g4 ..
  const int lc = CB == 16 ? unit * 2 + (g4 & 1) : (unit >> 1) * 4 + g4;
  int boff[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int s0 = CB == 16 ? 2 * ks : ks;
    int t = tap_of_slot(CB, MODE, s0);
    if (CB == 16) {
      const int t1 = tap_of_slot(CB, MODE, s0 + 1);
      t = (g4 >> 1) ? (t1 >= 0 ? t1 : t) : t;  // (an empty half reads the other one's pixel; its value is zeroed)
    }
    const int pt = MODE == DGRAD1 ? 8 - t : t;  // (stride-1 data gradient: tap t reads the pixel of tap 8 - t)
    const int kh = pt / 3, kw = pt - kh * 3;
    const int slot = MODE == DGRAD2 ? (kh == 0) * P + l16 + (kw == 0) : kh * P + l16 * ST + kw;
    boff[ks] = slot_addr(slot, lc, sb, ncm);
  }
  const int ch = c0 + unit * 16 + 4 * g4;  // the lane's 4 output channels
  float bv[4] = {0.f, 0.f, 0.f, 0.f};
  if (MODE == FWD && bias) {
#pragma unroll
    for (int j = 0; j < 4; ++j) bv[j] = bias[ch + j];
  }
  const char *sbase = reinterpret_cast<const char *>(src + c0);
  const uint32_t sbytes = a.s_bytes - static_cast<uint32_t>(c0) * 2u;

  // one fragment: K-steps [k0, k0 + nk) at halo row offset rb, stored at pixel (h, wd) of image n
  auto fragment = [&](auto k0c, auto nkc, int rb, int n, int h, int wd) __attribute__((always_inline)) {
    constexpr int k0 = decltype(k0c)::value, nk = decltype(nkc)::value;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = k0; ks < k0 + nk; ++ks) {
      uint4 q = *reinterpret_cast<const uint4 *>(halo + rb + boff[ks]);
      if (CB == 16 && tap_of_slot(CB, MODE, 2 * ks + 1) < 0 && g4 >= 2) q = make_uint4(0, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], __builtin_bit_cast(bf16x8, q), acc, 0, 0, 0);
    }
    if (h < a.Hd && wd < a.Wd) {
      bf16_t *out = dst + ((static_cast<size_t>(n) * a.Hd + h) * a.Wd + wd) * a.ps_d + ch;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = acc[j] + bv[j];
      if (MODE == FWD) {
        if (flag) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
        }
      } else if (flag) {  // relu(z) of the node, read by the lane that overwrites it
        const uint2 z = *reinterpret_cast<const uint2 *>(out);
        v[0] = __uint_as_float(z.x << 16) > 0.f ? v[0] : 0.f;
        v[1] = __uint_as_float(z.x & 0xffff0000u) > 0.f ? v[1] : 0.f;
        v[2] = __uint_as_float(z.y << 16) > 0.f ? v[2] : 0.f;
        v[3] = __uint_as_float(z.y & 0xffff0000u) > 0.f ? v[3] : 0.f;
      }
      *reinterpret_cast<uint2 *>(out) = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
    }
  };

  for (uint32_t it = blockIdx.x; it < a.items; it += gridDim.x) {
    int n, ph, pw;
    item_of(a, it, n, ph, pw);
    __syncthreads();  // the previous patch's readers are done
    const int oy = MODE == DGRAD2 ? ph * T::ROWS : ph * T::ROWS * S + T::OFF;
    const int ox = MODE == DGRAD2 ? pw * 16 : pw * 16 * S + T::OFF;
    stage<T::HR, T::HC, P>(halo, sbase, sbytes, n, oy, ox, a.Hs, a.Ws, a.ps_s, NU, wave, lane);
    wait_vmcnt<0>();
    __syncthreads();
    for (int r = fg; r < T::ROWS; r += FG) {
      if constexpr (MODE == DGRAD2) {
        static_for<4>([&](auto cc) {
          constexpr int cls = decltype(cc)::value;
          fragment(std::integral_constant<int, cls_first(CB, cls)>{}, std::integral_constant<int, cls_count(CB, cls)>{},
                   r * P * sb, n, ph * T::PH + 2 * r + (cls >> 1), pw * T::PW + 2 * l16 + (cls & 1));
        });
      } else {
        fragment(std::integral_constant<int, 0>{}, std::integral_constant<int, KS>{}, r * S * P * sb, n,
                 ph * T::PH + r, pw * T::PW + l16);
      }
    }
  }
}

// ---------------------------------------------------------------------------- weight gradient
// slab p of ws: [C][9][cg] partial dw of patches [p ipb, min(items, (p + 1) ipb))
template <int CB, int S>
__global__ __launch_bounds__(NT) void gconv_wgrad_partial(const bf16_t *__restrict__ x, const bf16_t *__restrict__ dy,
                                                          float *__restrict__ ws, const GArgs a, uint32_t ipb) {
  using T = Tile<S, FWD>;
  constexpr int P = T::P, R = T::ROWS, PJ = CB == 16 ? 1 : 2;
  constexpr int DYB = R * 16 * 128;
  __shared__ __attribute__((aligned(1024))) char smem[T::HALO + DYB];
  char *halo = smem, *dyb = smem + T::HALO;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l16 = lane & 15, g4 = lane >> 4;
  const int NU = a.NU, sb = NU * 32, ncm = 2 * NU - 1;
  const int c0 = blockIdx.y * NU * 16;
  const int npair = CB == 16 ? NU : 2 * NU;  // (output unit, input unit) pairs of the slice's blocks

  // transposed reads: lane (i = l16, g4) reads pixel 8 g4 + i / 4 (and + 4) of the K-step's 32,
  // channels 4 (i % 4) .. + 3 of the unit
  const int kq = 8 * g4 + (l16 >> 2);
  const int prow = kq >> 4, pcol = kq & 15;  // (kq + 4 lies in the same patch row)
  const int cbyte = (l16 & 3) * 8;           // byte of the lane's 4 channels within the unit's 32
  int cou[PJ], ciu[PJ], offA[PJ][2], offB[PJ][3][2];
  bool live[PJ];
#pragma unroll
  for (int j = 0; j < PJ; ++j) {
    const int p = wave + 4 * j;
    live[j] = p < npair;
    const int pp = live[j] ? p : 0;
    cou[j] = CB == 16 ? pp : 2 * (pp >> 2) + ((pp >> 1) & 1);
    ciu[j] = CB == 16 ? pp : 2 * (pp >> 2) + (pp & 1);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int col = pcol + 4 * h;
      offA[j][h] = slot_addr(prow * 16 + col, cou[j] * 2 + (cbyte >> 4), sb, ncm) + (cbyte & 15);
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
        offB[j][kw][h] = slot_addr(prow * S * P + col * S + kw, ciu[j] * 2 + (cbyte >> 4), sb, ncm) + (cbyte & 15);
    }
  }
  f32x4 acc[PJ][9];
#pragma unroll
  for (int j = 0; j < PJ; ++j)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const char *xbase = reinterpret_cast<const char *>(x + c0);
  const char *dbase = reinterpret_cast<const char *>(dy + c0);
  const uint32_t xbytes = a.s_bytes - static_cast<uint32_t>(c0) * 2u;
  const uint32_t dbytes = a.d_bytes - static_cast<uint32_t>(c0) * 2u;
  const uint32_t it0 = blockIdx.x * ipb;
  const uint32_t it1 = it0 + ipb < a.items ? it0 + ipb : a.items;
  for (uint32_t it = it0; it < it1; ++it) {
    int n, ph, pw;
    item_of(a, it, n, ph, pw);
    __syncthreads();  // the previous patch's readers are done
    stage<T::HR, T::HC, P>(halo, xbase, xbytes, n, ph * R * S - 1, pw * 16 * S - 1, a.Hs, a.Ws, a.ps_s, NU, wave, lane);
    stage<R, 16, 16>(dyb, dbase, dbytes, n, ph * R, pw * 16, a.Hd, a.Wd, a.ps_d, NU, wave, lane);
    wait_vmcnt<0>();
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < R / 2; ++kk) {
#pragma unroll
      for (int j = 0; j < PJ; ++j) {
        if (!live[j]) continue;  // wave-uniform
        const char *pa = dyb + kk * 32 * sb;
        const bf16x8 fa = frag_tr(pa + offA[j][0], pa + offA[j][1]);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int kh = t / 3, kw = t % 3;
          const char *pb = halo + (2 * kk * S + kh) * P * sb;
          const bf16x8 fb = frag_tr(pb + offB[j][kw][0], pb + offB[j][kw][1]);
          acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc[j][t], 0, 0, 0);
        }
      }
    }
  }
  // acc[j][t][m]: output channel 4 g4 + m of unit cou, input channel l16 of unit ciu; kept where
  // the two share a group
  float *slab = ws + static_cast<size_t>(blockIdx.x) * a.C * 9 * a.cg;
#pragma unroll
  for (int j = 0; j < PJ; ++j) {
    if (!live[j]) continue;
    const int ci_b = CB == 16 ? l16 : (ciu[j] & 1) * 16 + l16;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int co_u = 4 * g4 + m;
      const int co_b = CB == 16 ? co_u : (cou[j] & 1) * 16 + co_u;
      if ((co_b >> a.lg) != (ci_b >> a.lg)) continue;
      const size_t co = static_cast<size_t>(c0) + cou[j] * 16 + co_u;
#pragma unroll
      for (int t = 0; t < 9; ++t) slab[(co * 9 + t) * a.cg + (ci_b & (a.cg - 1))] = acc[j][t][m];
    }
  }
}

// dw[e] += sum over the slabs: ML lanes per element each sum a run of consecutive slabs in slab
// order, lane 0 then sums the lanes in lane order (the merge of dwconv_kernels.hip)
constexpr int ML = 16, MC = NT / ML;
__global__ __launch_bounds__(NT) void gconv_wgrad_merge(const float *__restrict__ ws, int P, long slab, float *dw, int nw) {
  __shared__ float s_sum[ML][MC];
  const int el = threadIdx.x % MC, ln = threadIdx.x / MC;
  const int e = blockIdx.x * MC + el;
  const int chunk = (P + ML - 1) / ML;
  const int p0 = ln * chunk, p1 = p0 + chunk < P ? p0 + chunk : P;
  float sum = 0.f;
  if (e < nw) {
#pragma unroll 8
    for (int p = p0; p < p1; ++p) sum += ws[static_cast<size_t>(p) * slab + e];
  }
  s_sum[ln][el] = sum;
  __syncthreads();
  if (ln != 0 || e >= nw) return;
  for (int q = 1; q < ML; ++q) sum += s_sum[q][el];
  dw[e] += sum;
}

// what the kernels serve; Ho / Wo by the layer's rule
static bool serves(int N, int H, int W, int C, int Cout, int groups, int KH, int KW, int stride, int pad_y, int pad_x,
                   int &cg, int &Ho, int &Wo) {
  if (N < 1 || H < 1 || W < 1 || groups < 4 || C != Cout || C % groups || C % 16) return false;
  cg = C / groups;
  if (cg != 4 && cg != 8 && cg != 16 && cg != 32) return false;
  if (KH != 3 || KW != 3 || pad_y != 1 || pad_x != 1 || (stride != 1 && stride != 2)) return false;
  Ho = (H - 1) / stride + 1;
  Wo = (W - 1) / stride + 1;
  return true;
}

// byte extent of an NHWC view of C channels with pixel stride ps; 0: not addressable in 31 bits
static uint32_t extent(long npix, long ps, int C) {
  const long b = ((npix - 1) * ps + C) * 2;
  return b < (1L << 31) ? static_cast<uint32_t>(b) : 0u;
}

// Hs x Ws: staged tensor, Hd x Wd: walked tensor, in patches of ph x pw
static bool make_args(GArgs &a, int N, int Hs, int Ws, int Hd, int Wd, int C, int cg, long ps_s, long ps_d, int ph,
                      int pw) {
  a.N = N; a.Hs = Hs; a.Ws = Ws; a.Hd = Hd; a.Wd = Wd; a.C = C; a.cg = cg;
  a.lg = cg == 4 ? 2 : (cg == 8 ? 3 : (cg == 16 ? 4 : 5));
  a.NU = C % 64 == 0 ? 4 : (C % 32 == 0 ? 2 : 1);
  a.ps_s = ps_s; a.ps_d = ps_d;
  a.s_bytes = extent(static_cast<long>(N) * Hs * Ws, ps_s, C);
  a.d_bytes = extent(static_cast<long>(N) * Hd * Wd, ps_d, C);
  if (!a.s_bytes || !a.d_bytes) return false;
  const long tw = (Wd + pw - 1) / pw, th = (Hd + ph - 1) / ph;
  const long items = static_cast<long>(N) * th * tw;
  if (items >= (1L << 31) - BLOCKS) return false;  // (32-bit item walk)
  a.items = static_cast<uint32_t>(items);
  a.tw = static_cast<uint32_t>(tw);
  a.thw = static_cast<uint32_t>(th * tw);
  a.dtw = make_fastdiv(a.tw);
  a.dthw = make_fastdiv(a.thw);
  return true;
}

static dim3 walk_grid(const GArgs &a) {
  const int ny = a.C / (a.NU * 16);
  const long cap = BLOCKS / ny > 1 ? BLOCKS / ny : 1;
  const long nb = a.items < cap ? a.items : cap;
  return dim3(static_cast<unsigned>(nb), static_cast<unsigned>(ny));
}

static bool operands_ok(const void *p, long ps, const void *q, long qs, int C) {
  return ps >= C && qs >= C && ps % 8 == 0 && qs % 8 == 0 && aligned16(p) && aligned16(q);
}

#define CXN_GC_MM(CB_, ST_, MODE_)                                                                                  \
  CXN_LAUNCH((gconv_mm<CB_, ST_, MODE_>), grid, NT, 0, S_, (const bf16_t *)src, (const bf16_t *)w, bias, (bf16_t *)dst, \
             a, flag)

}  // namespace


// y = [relu](conv(x, w) + bias); xs / ys: pixel strides in elements; bias nullable.
CXN_API int cxn_gconv_fwd(const void *x, long xs, const void *w, const float *bias, void *y, long ys, int N, int H,
                          int W, int C, int Cout, int groups, int KH, int KW, int stride, int pad_y, int pad_x,
                          int relu, void *stream) {
  int cg, Ho, Wo;
  if (!serves(N, H, W, C, Cout, groups, KH, KW, stride, pad_y, pad_x, cg, Ho, Wo)) return -1;
  if (!operands_ok(x, xs, y, ys, C) || !aligned16(w)) return -1;
  GArgs a;
  const int rows = stride == 1 ? Tile<1, FWD>::PH : Tile<2, FWD>::PH;
  if (!make_args(a, N, H, W, Ho, Wo, C, cg, xs, ys, rows, 16)) return -1;
  const dim3 grid = walk_grid(a);
  const void *src = x;
  void *dst = y;
  const int flag = relu;
  if (cg == 32) {
    if (stride == 1) CXN_GC_MM(32, 1, FWD);
    else CXN_GC_MM(32, 2, FWD);
  } else {
    if (stride == 1) CXN_GC_MM(16, 1, FWD);
    else CXN_GC_MM(16, 2, FWD);
  }
  RET;
}

// dx [N][H][W][C] = conv_transpose(dy, w), every element written; H, W: the forward input size (at
// stride 2 two sizes give the same Ho, Wo).  mask_relu: dx holds relu(z) on entry and the result is
// exactly 0 where that is not > 0.
CXN_API int cxn_gconv_bwd_data(const void *dy, long dys, const void *w, void *dx, long dxs, int N, int H, int W,
                               int C, int Cout, int groups, int KH, int KW, int stride, int pad_y, int pad_x,
                               int mask_relu, void *stream) {
  int cg, Ho, Wo;
  if (!serves(N, H, W, C, Cout, groups, KH, KW, stride, pad_y, pad_x, cg, Ho, Wo)) return -1;
  if (!operands_ok(dy, dys, dx, dxs, C) || !aligned16(w)) return -1;
  GArgs a;
  const int ph = stride == 1 ? Tile<1, DGRAD1>::PH : Tile<2, DGRAD2>::PH;
  const int pw = stride == 1 ? Tile<1, DGRAD1>::PW : Tile<2, DGRAD2>::PW;
  if (!make_args(a, N, Ho, Wo, H, W, C, cg, dys, dxs, ph, pw)) return -1;
  const dim3 grid = walk_grid(a);
  const void *src = dy;
  void *dst = dx;
  const float *bias = nullptr;
  const int flag = mask_relu;
  if (cg == 32) {
    if (stride == 1) CXN_GC_MM(32, 1, DGRAD1);
    else CXN_GC_MM(32, 2, DGRAD2);
  } else {
    if (stride == 1) CXN_GC_MM(16, 1, DGRAD1);
    else CXN_GC_MM(16, 2, DGRAD2);
  }
  RET;
}

// dw [Cout][3][3][cg] fp32 += sum over pixels of dy (x) x.  ws: fp32 workspace of ws_floats >=
// P C 9 cg, P the slab count below (mirrored by ops.gemm.gconv_wgrad_partials); -2 when it is smaller.
CXN_API int cxn_gconv_bwd_weight(const void *x, long xs, const void *dy, long dys, float *dw, float *ws, long ws_floats,
                                 int N, int H, int W, int C, int Cout, int groups, int KH, int KW, int stride,
                                 int pad_y, int pad_x, void *stream) {
  int cg, Ho, Wo;
  if (!serves(N, H, W, C, Cout, groups, KH, KW, stride, pad_y, pad_x, cg, Ho, Wo)) return -1;
  if (!operands_ok(x, xs, dy, dys, C)) return -1;
  GArgs a;
  const int rows = stride == 1 ? Tile<1, FWD>::PH : Tile<2, FWD>::PH;
  if (!make_args(a, N, H, W, Ho, Wo, C, cg, xs, dys, rows, 16)) return -1;
  const int ny = C / (a.NU * 16);
  const long pmax = PMAX / ny > 1 ? PMAX / ny : 1;
  const long ipb = (static_cast<long>(a.items) + pmax - 1) / pmax;
  const int P = static_cast<int>((static_cast<long>(a.items) + ipb - 1) / ipb);
  const long slab = static_cast<long>(C) * 9 * cg;
  if (!ws || static_cast<long>(P) * slab > ws_floats) return -2;
  const dim3 grid(static_cast<unsigned>(P), static_cast<unsigned>(ny));
#define CXN_GC_WG(CB_, ST_)                                                                                         \
  CXN_LAUNCH((gconv_wgrad_partial<CB_, ST_>), grid, NT, 0, S_, (const bf16_t *)x, (const bf16_t *)dy, ws, a,         \
             static_cast<uint32_t>(ipb))
  if (cg == 32) {
    if (stride == 1) CXN_GC_WG(32, 1);
    else CXN_GC_WG(32, 2);
  } else {
    if (stride == 1) CXN_GC_WG(16, 1);
    else CXN_GC_WG(16, 2);
  }
#undef CXN_GC_WG
  const int nw = static_cast<int>(slab);
  CXN_LAUNCH((gconv_wgrad_merge), (nw + MC - 1) / MC, NT, 0, S_, (const float *)ws, P, slab, dw, nw);
  RET;
}
