// Large-kernel depthwise convolution (7 x 7, 9 x 9, 11 x 11; ConvNeXt's token mixer) as LDS stencils.
// dwconv_kernels.hip keeps a lane's K K x 8 weights in registers, which stops at 5 x 5: 49 packed
// vectors and the accumulators do not fit.  Here the block's input halo and its weights live in LDS
// and a lane holds one kernel row of weights at a time.
//
//   cxn_dwlk_fwd         y  = [relu](dwconv(x, w) + bias)
//   cxn_dwlk_bwd_data    dx = dwconv_transpose(dy, w) [masked by relu'(z), dx = relu(z) on entry]
//   cxn_dwlk_bwd_weight  dw += sum over pixels of dy x;  db += sum of dy     (two launches)
//
// Served: groups == C == Cout, C % 8 == 0, KH == KW in {7, 9, 11}, stride 1, pad_y and pad_x in
// [0, K) independently; everything else returns -1.  Activations are NHWC bf16 with an explicit
// pixel stride in elements (a node may be a channel slice of a wider buffer), weights
// [C][K][K][1] bf16, accumulation fp32, one rounding.
//
// Geometry.  A block of 256 lanes owns a patch of TH x TW pixels of the tensor it walks (forward:
// y, data gradient: dx, weight gradient: dy) times CG groups of 8 channels:
//     Big    16 x 16 pixels x  8 groups ( 64 channels), a lane computes 2 x 4 pixels
//     Small   8 x  8 pixels x 16 groups (128 channels), a lane computes 2 x 2 pixels
// Small serves maps of at most 8 x 8 (ConvNeXt's 7 x 7 stage: one patch per image, 49 of a patch's
// 64 pixels inside the map instead of 49 of 256); everything else is Big.  The two shapes are a
// design choice from counting lanes and LDS bytes; other patch shapes have not been timed.  The halo of the patch,
// (TH + K - 1) x (TW + K - 1) pixels x CG groups, is staged once per patch by LDS-DMA, 16 bytes per
// lane; a pixel outside the image, or a group past C, is a load past the buffer's records, which
// writes zeros: borders cost no branch and no padded copy (gconv_kernels.hip's scheme).  The K K
// weight vectors of the block's channels are transposed into LDS once per block ([tap][group],
// 16 bytes each; the data gradient stores them in reverse tap order, so at stride 1 it is the
// forward stencil with pads K - 1 - p and w itself, no flipped copy).
//
// LDS layout and bank conflicts.  A halo pixel is a slot of 16 CG bytes (group gl at byte 16 gl),
// slots in rows of an odd pitch HP = TW + K.  Lane t is group t % CG, pixel lane t / CG.  At
// CG = 16 any 16 consecutive lanes read the 16 groups of one slot: 256 consecutive bytes, all 64
// banks once.  At CG = 8 they are 8 groups x 2 neighbouring pixel lanes, whose columns differ by 4
// (stencil) or whose rows differ by an odd number (weight gradient): column c is stored at
// c ^ ((c >> 2) & 1), so the two slots differ in the parity of their index either way (odd pitch)
// and the 16 lanes again cover 256 distinct bytes mod 256.  Every LDS read is 16 bytes.  A weight
// vector is read by all pixel lanes of a group at one address: a broadcast.
//
// Stencil.  For each kernel row kh the lane reads its K weight vectors (the only weights live in
// registers), then for each of its RH output rows the RW + K - 1 halo vectors of row i + kh, each
// feeding up to RW pixels.  The halo is not double-buffered inside a block: at K = 7 two blocks fit a
// CU (70 KB each) and the intent is that one stages while the other computes -- whether they do
// overlap has not been observed in a trace.  Measured (docs/performance.md): the stencil runs at
// 0.9 - 1.0 TB/s of map bytes on ConvNeXt-T's 56^2 .. 14^2 sites, 4 - 5 times the time of a copy of
// the same bytes: it is bound by its fp32 FMAs and bf16 unpacking, not by memory or staging.
//
// Weight gradient.  K K x 8 accumulators do not fit a lane, so a lane owns one kernel row kh of one
// group (K x 8 accumulators) and a strip of the patch's rows (row = strip, strip + NS, ..; NS =
// lanes per group / K strips).  It walks a row of the x halo from left to right with a window of the
// last K dy vectors in registers: one x read and one dy read feed K x 8 FMAs.  The dy patch is
// staged like the halo (rows and columns of dy past the map are zeros).  The strips of a block are
// summed through LDS in strip order into a slab of fp32 partials, and the second launch merges the
// slabs in a fixed order (dw_wgrad_merge.h).  No atomics: the same bits on every run.  At K = 7 the
// Big shape keeps 28 of a group's 32 lanes busy and one block per CU (100 KB of LDS); measured at
// 1.7 - 2.1 times the stencil's time, untuned.
#include "gfx950_prims.h"

using namespace cxg;

namespace {

constexpr int NT = 256;
constexpr int PMAX = 512;     // weight gradient: slabs to aim for (over all channel blocks)
constexpr int BLOCKS = 1024;  // forward / data gradient: blocks to aim for
constexpr uint32_t PAST = 0x80000000u;  // >= num_records: the load returns zeros
constexpr int SMALL_MAP = 8;  // maps up to SMALL_MAP x SMALL_MAP take the Small patch

constexpr int kib(int b) { return (b + 1023) / 1024 * 1024; }

template <int K_, int TH_, int TW_, int RH_, int RW_>
struct Cfg {
  static constexpr int K = K_, TH = TH_, TW = TW_, RH = RH_, RW = RW_;
  static constexpr int PXL = TW / RW;             // pixel lanes along W
  static constexpr int LPG = (TH / RH) * PXL;     // lanes per channel group
  static constexpr int CG = NT / LPG;             // channel groups per block
  static constexpr int SLOT = CG * 16;            // bytes per pixel
  static constexpr bool SWZ = CG < 16;
  static constexpr int HR = TH + K - 1, HC = TW + K - 1, HP = HC | 1;
  static constexpr int HALO = kib(HR * HP * SLOT);
  static constexpr int WL = K * K * SLOT;
  static constexpr int DP = TW | 1;               // the weight gradient's dy patch
  static constexpr int DYB = kib(TH * DP * SLOT);
  static constexpr int NS = LPG / K;              // and its row strips
  static constexpr int RED = NT * (K + 1) * 8 * 4;
  static constexpr int WG_LDS = HALO + DYB > RED ? HALO + DYB : RED;
  static_assert(HC % 2 == 0 && NS >= 1 && TH % RH == 0 && TW % RW == 0 && (CG & (CG - 1)) == 0, "patch shape");
};
template <int K> using Big = Cfg<K, 16, 16, 2, 4>;
template <int K> using Small = Cfg<K, 8, 8, 2, 2>;

struct LArgs {
  int N, Hs, Ws;      // the staged tensor (forward / weight gradient: x; data gradient: dy)
  int Hd, Wd;         // the tensor the patches walk (forward: y; data gradient: dx; weight gradient: dy)
  int G;              // groups of 8 channels
  int oy, ox;         // the halo's origin relative to the patch's first pixel
  long ps_s, ps_d;    // pixel strides in elements
  uint32_t s_bytes, d_bytes;  // byte extents of the two views, < 2^31
  uint32_t items, tw, thw;    // patches, patches per row, patches per image
  FastDiv dtw, dthw;
};

__device__ __forceinline__ void item_of(const LArgs &a, uint32_t it, int &n, int &ph, int &pw) {
  const uint32_t nn = fdiv(it, a.dthw);
  const uint32_t rem = it - nn * a.thw;
  const uint32_t hh = fdiv(rem, a.dtw);
  n = static_cast<int>(nn);
  ph = static_cast<int>(hh);
  pw = static_cast<int>(rem - hh * a.tw);
}

// stored column of logical column c
template <bool SWZ>
__device__ __forceinline__ constexpr int col_of(int c) {
  return SWZ ? c ^ ((c >> 2) & 1) : c;
}

// Stage HR x HC pixels (rows of HP slots, CG groups per slot) of image n from pixel (oy, ox) of an
// H x W tensor on: 1-KiB LDS-DMA groups, lane -> 16-byte chunk 64 q + lane of the region.  Chunks
// outside the image, past the halo or of a group >= live get zeros.
template <int HR, int HC, int HP, int CG, bool SWZ>
__device__ __forceinline__ void stage(char *dst, const char *base, uint32_t nbytes, int n, int oy, int ox, int H,
                                      int W, long ps, int live, int wave, int lane) {
  constexpr int NG = (HR * HP * CG + 63) / 64;
  for (int q = wave; q < NG; q += NT / 64) {
    const int ch = q * 64 + lane;
    const int slot = ch / CG, pg = ch % CG;
    const int hr = slot / HP, hc = col_of<SWZ>(slot - hr * HP);
    const int gh = oy + hr, gw = ox + hc;
    const bool ok = hr < HR && hc < HC && pg < live && static_cast<unsigned>(gh) < static_cast<unsigned>(H) &&
                    static_cast<unsigned>(gw) < static_cast<unsigned>(W);
    uint32_t off = ok ? static_cast<uint32_t>((n * H + gh) * W + gw) * static_cast<uint32_t>(ps) * 2u + pg * 16u : PAST;
    asm volatile("" : "+v"(off));  // keep the select: no per-lane branch around the DMA
    lds_dma16(base, nbytes, dst + q * 1024, off);
  }
}

// ------------------------------------------------------- forward and data gradient (one stencil)
// REV: the taps in reverse order (data gradient); flag: relu (forward) / mask_relu (data gradient)
template <class T, bool REV>
__global__ __launch_bounds__(NT) void dwlk_stencil(const bf16_t *__restrict__ src, const bf16_t *__restrict__ w,
                                                   const float *__restrict__ bias, bf16_t *dst, const LArgs a,
                                                   int flag) {
  constexpr int K = T::K, KK = K * K, CG = T::CG, RH = T::RH, RW = T::RW;
  __shared__ __attribute__((aligned(1024))) char smem[T::HALO + T::WL];
  char *halo = smem, *wl = smem + T::HALO;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int gl = t % CG, pl = t / CG;
  const int py = pl / T::PXL, px = pl - py * T::PXL;
  const int g0 = blockIdx.y * CG;
  const int live = a.G - g0 < CG ? a.G - g0 : CG;
  const size_t c0 = static_cast<size_t>(g0 + gl) * 8;

  for (int e = t; e < KK * CG; e += NT) {  // [C][K K] -> [tap][group] vectors of 8 channels
    const int tap = e / CG, g = e - tap * CG;
    uint32_t h[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = g < live ? w[(static_cast<size_t>(g0 + g) * 8 + j) * KK + tap] : 0u;
    const int dt = REV ? KK - 1 - tap : tap;
    *reinterpret_cast<uint4 *>(wl + (dt * CG + g) * 16) =
        make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
  }
  float bv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bv[j] = (!REV && bias && gl < live) ? bias[c0 + j] : 0.f;
  const char *sbase = reinterpret_cast<const char *>(src + static_cast<size_t>(g0) * 8);
  const uint32_t sbytes = a.s_bytes - static_cast<uint32_t>(g0) * 16u;

  for (uint32_t it = blockIdx.x; it < a.items; it += gridDim.x) {
    int n, ph, pw;
    item_of(a, it, n, ph, pw);
    __syncthreads();  // the previous patch's readers are done
    stage<T::HR, T::HC, T::HP, CG, T::SWZ>(halo, sbase, sbytes, n, ph * T::TH + a.oy, pw * T::TW + a.ox, a.Hs, a.Ws,
                                           a.ps_s, live, wave, lane);
    wait_vmcnt<0>();
    __syncthreads();  // (the first patch: the weights as well)
    float acc[RH][RW][8];
#pragma unroll
    for (int i = 0; i < RH; ++i)
#pragma unroll
      for (int p = 0; p < RW; ++p)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][p][j] = bv[j];
#pragma unroll 1
    for (int kh = 0; kh < K; ++kh) {
      float wf[K][8];
#pragma unroll
      for (int kw = 0; kw < K; ++kw)
        unpack8(*reinterpret_cast<const uint4 *>(wl + ((kh * K + kw) * CG + gl) * 16), wf[kw]);
#pragma unroll
      for (int i = 0; i < RH; ++i) {
        const char *row = halo + ((py * RH + i + kh) * T::HP * CG + gl) * 16;
#pragma unroll
        for (int m = 0; m < RW + K - 1; ++m) {
          float xf[8];
          unpack8(*reinterpret_cast<const uint4 *>(row + col_of<T::SWZ>(px * RW + m) * T::SLOT), xf);
#pragma unroll
          for (int p = 0; p < RW; ++p) {
            const int kw = m - p;
            if (kw >= 0 && kw < K) {
#pragma unroll
              for (int j = 0; j < 8; ++j) acc[i][p][j] = fmaf(xf[j], wf[kw][j], acc[i][p][j]);
            }
          }
        }
      }
    }
    if (gl < live) {
#pragma unroll
      for (int i = 0; i < RH; ++i) {
#pragma unroll
        for (int p = 0; p < RW; ++p) {
          const int h = ph * T::TH + py * RH + i, wd = pw * T::TW + px * RW + p;
          if (h < a.Hd && wd < a.Wd) {
            bf16_t *out = dst + ((static_cast<size_t>(n) * a.Hd + h) * a.Wd + wd) * a.ps_d + c0;
            if (flag) {
              if (REV) {  // relu(z) of the node, read by the lane that overwrites it
                float zf[8];
                unpack8(*reinterpret_cast<const uint4 *>(out), zf);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][p][j] = zf[j] > 0.f ? acc[i][p][j] : 0.f;
              } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][p][j] = fmaxf(acc[i][p][j], 0.f);
              }
            }
            *reinterpret_cast<uint4 *>(out) = pack8(acc[i][p]);
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------- weight gradient
// slab p of ws: [C][K K] partial dw, then [C] partial db, of patches [p ipb, min(items, (p + 1) ipb))
template <class T>
__global__ __launch_bounds__(NT) void dwlk_wgrad_partial(const bf16_t *__restrict__ x, const bf16_t *__restrict__ dy,
                                                         float *__restrict__ ws, const LArgs a, uint32_t ipb, int C) {
  constexpr int K = T::K, KK = K * K, CG = T::CG, TW = T::TW;
  __shared__ __attribute__((aligned(1024))) char smem[T::WG_LDS];
  char *halo = smem, *dyl = smem + T::HALO;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int gl = t % CG, role = t / CG;
  const int strip = role / K, kh = role - strip * K;
  const int g0 = blockIdx.y * CG;
  const int live = a.G - g0 < CG ? a.G - g0 : CG;
  const char *xbase = reinterpret_cast<const char *>(x + static_cast<size_t>(g0) * 8);
  const char *dbase = reinterpret_cast<const char *>(dy + static_cast<size_t>(g0) * 8);
  const uint32_t xbytes = a.s_bytes - static_cast<uint32_t>(g0) * 16u;
  const uint32_t dbytes = a.d_bytes - static_cast<uint32_t>(g0) * 16u;
  float acc[K][8], accb[8];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) accb[j] = 0.f;
  const float first = kh == 0 ? 1.f : 0.f;  // the kh = 0 lanes also sum dy (each dy vector once)

  const uint32_t it0 = blockIdx.x * ipb;
  const uint32_t it1 = it0 + ipb < a.items ? it0 + ipb : a.items;
  for (uint32_t it = it0; it < it1; ++it) {
    int n, ph, pw;
    item_of(a, it, n, ph, pw);
    __syncthreads();  // the previous patch's readers are done
    stage<T::HR, T::HC, T::HP, CG, T::SWZ>(halo, xbase, xbytes, n, ph * T::TH + a.oy, pw * TW + a.ox, a.Hs, a.Ws,
                                           a.ps_s, live, wave, lane);
    stage<T::TH, TW, T::DP, CG, T::SWZ>(dyl, dbase, dbytes, n, ph * T::TH, pw * TW, a.Hd, a.Wd, a.ps_d, live, wave,
                                        lane);
    wait_vmcnt<0>();
    __syncthreads();
    if (strip < T::NS) {
#pragma unroll 1
      for (int r = strip; r < T::TH; r += T::NS) {
        const char *xrow = halo + ((r + kh) * T::HP * CG + gl) * 16;
        const char *drow = dyl + (r * T::DP * CG + gl) * 16;
        float win[K][8];  // dy at columns xi - K + 1 .. xi of the row, column c in win[c % K]
        static_for<T::HC>([&](auto xc) {
          constexpr int xi = decltype(xc)::value;
          if constexpr (xi < TW) {
            unpack8(*reinterpret_cast<const uint4 *>(drow + col_of<T::SWZ>(xi) * T::SLOT), win[xi % K]);
#pragma unroll
            for (int j = 0; j < 8; ++j) accb[j] = fmaf(first, win[xi % K][j], accb[j]);
          }
          float xf[8];
          unpack8(*reinterpret_cast<const uint4 *>(xrow + col_of<T::SWZ>(xi) * T::SLOT), xf);
#pragma unroll
          for (int kw = 0; kw < K; ++kw) {
            const int wo = xi - kw;  // the dy column this x column meets at tap kw
            if (wo >= 0 && wo < TW) {
#pragma unroll
              for (int j = 0; j < 8; ++j) acc[kw][j] = fmaf(xf[j], win[wo % K][j], acc[kw][j]);
            }
          }
        });
      }
    }
  }
  // the strips of each (group, kernel row), summed in strip order; lane t's K x 8 sums at float
  // 8 K t, its dy sums behind them at 8 K NT + 8 t
  __syncthreads();
  float *red = reinterpret_cast<float *>(smem);
#pragma unroll
  for (int k = 0; k <= K; ++k) {
    const float *v = k < K ? acc[k % K] : accb;
    float *p = k < K ? red + (t * K + k) * 8 : red + NT * K * 8 + t * 8;
    *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4 *>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
  __syncthreads();
  float *slab = ws + static_cast<size_t>(blockIdx.x) * C * (KK + 1);
  for (int e = t; e < CG * (KK + 1) * 8; e += NT) {
    const int j = e & 7, q = e >> 3;
    const int g = q % CG, tap = q / CG;  // tap KK: the dy sums
    if (g >= live) continue;
    const int rk = tap < KK ? tap / K : 0, kw = tap < KK ? tap - rk * K : 0;
    float sum = 0.f;
    for (int s = 0; s < T::NS; ++s) {
      const int lt = (s * K + rk) * CG + g;
      sum += tap < KK ? red[(lt * K + kw) * 8 + j] : red[NT * K * 8 + lt * 8 + j];
    }
    const size_t c = static_cast<size_t>(g0 + g) * 8 + j;
    slab[tap < KK ? c * KK + tap : static_cast<size_t>(C) * KK + c] = sum;
  }
}

#include "dw_wgrad_merge.h"  // dwconv_wgrad_merge: dw += the slabs in a fixed order

// what the kernels serve; Ho / Wo by the layer's rule
static bool serves(int N, int H, int W, int C, int Cout, int groups, int KH, int KW, int stride, int pad_y, int pad_x,
                   int &Ho, int &Wo) {
  if (N < 1 || H < 1 || W < 1 || C < 8 || C % 8 || groups != C || Cout != C) return false;
  if (KH != KW || (KH != 7 && KH != 9 && KH != 11) || stride != 1) return false;
  if (pad_y < 0 || pad_y >= KH || pad_x < 0 || pad_x >= KW) return false;
  if (H + 2 * pad_y < KH || W + 2 * pad_x < KW) return false;
  Ho = H + 2 * pad_y - KH + 1;
  Wo = W + 2 * pad_x - KW + 1;
  return true;
}

// byte extent of an NHWC view of C channels with pixel stride ps; 0: not addressable in 31 bits
static uint32_t extent(long npix, long ps, int C) {
  const long b = ((npix - 1) * ps + C) * 2;
  return b < (1L << 31) ? static_cast<uint32_t>(b) : 0u;
}

static bool small_map(int Hd, int Wd) { return Hd <= SMALL_MAP && Wd <= SMALL_MAP; }

// Hs x Ws: staged tensor, Hd x Wd: walked tensor; (oy, ox): halo origin relative to a patch
static bool make_args(LArgs &a, int N, int Hs, int Ws, int Hd, int Wd, int C, long ps_s, long ps_d, int oy, int ox) {
  a.N = N; a.Hs = Hs; a.Ws = Ws; a.Hd = Hd; a.Wd = Wd; a.G = C / 8; a.oy = oy; a.ox = ox;
  a.ps_s = ps_s; a.ps_d = ps_d;
  a.s_bytes = extent(static_cast<long>(N) * Hs * Ws, ps_s, C);
  a.d_bytes = extent(static_cast<long>(N) * Hd * Wd, ps_d, C);
  if (!a.s_bytes || !a.d_bytes) return false;
  const int pt = small_map(Hd, Wd) ? Small<7>::TH : Big<7>::TH;  // (square patches)
  const long tw = (Wd + pt - 1) / pt, th = (Hd + pt - 1) / pt;
  const long items = static_cast<long>(N) * th * tw;
  if (items >= (1L << 31) - BLOCKS) return false;  // (32-bit item walk)
  a.items = static_cast<uint32_t>(items);
  a.tw = static_cast<uint32_t>(tw);
  a.thw = static_cast<uint32_t>(th * tw);
  a.dtw = make_fastdiv(a.tw);
  a.dthw = make_fastdiv(a.thw);
  return true;
}

static int channel_blocks(const LArgs &a) {
  const int cg = small_map(a.Hd, a.Wd) ? Small<7>::CG : Big<7>::CG;
  return (a.G + cg - 1) / cg;
}

static bool operands_ok(const void *p, long ps, const void *q, long qs, int C) {
  return ps >= C && qs >= C && ps % 8 == 0 && qs % 8 == 0 && aligned16(p) && aligned16(q);
}

static int launch_stencil(bool rev, int K, const void *src, const void *w, const float *bias, void *dst,
                          const LArgs &a, int flag, void *stream) {
  const int ny = channel_blocks(a);
  const long cap = BLOCKS / ny > 1 ? BLOCKS / ny : 1;
  const dim3 grid(static_cast<unsigned>(a.items < cap ? a.items : cap), static_cast<unsigned>(ny));
  const bool sm = small_map(a.Hd, a.Wd);
#define CXN_LK_ST(T_, REV_)                                                                                         \
  CXN_LAUNCH((dwlk_stencil<T_, REV_>), grid, NT, 0, S_, (const bf16_t *)src, (const bf16_t *)w, bias, (bf16_t *)dst, a, flag)
#define CXN_LK_ST_K(K_)                                                                                             \
  do {                                                                                                              \
    if (sm && rev) CXN_LK_ST(Small<K_>, true);                                                                      \
    else if (sm) CXN_LK_ST(Small<K_>, false);                                                                       \
    else if (rev) CXN_LK_ST(Big<K_>, true);                                                                         \
    else CXN_LK_ST(Big<K_>, false);                                                                                 \
  } while (0)
  if (K == 7) CXN_LK_ST_K(7);
  else if (K == 9) CXN_LK_ST_K(9);
  else CXN_LK_ST_K(11);
#undef CXN_LK_ST_K
#undef CXN_LK_ST
  RET;
}

}  // namespace


// y = [relu](dwconv(x, w) + bias); xs / ys: pixel strides in elements; bias nullable.
CXN_API int cxn_dwlk_fwd(const void *x, long xs, const void *w, const float *bias, void *y, long ys, int N, int H,
                         int W, int C, int Cout, int groups, int KH, int KW, int stride, int pad_y, int pad_x,
                         int relu, void *stream) {
  int Ho, Wo;
  if (!serves(N, H, W, C, Cout, groups, KH, KW, stride, pad_y, pad_x, Ho, Wo)) return -1;
  if (!operands_ok(x, xs, y, ys, C) || (reinterpret_cast<uintptr_t>(w) & 1)) return -1;
  LArgs a;
  if (!make_args(a, N, H, W, Ho, Wo, C, xs, ys, -pad_y, -pad_x)) return -1;
  return launch_stencil(false, KH, x, w, bias, y, a, relu, stream);
}

// dx [N][H][W][C] = dwconv_transpose(dy, w), every element written: the forward stencil over dy
// with the taps reversed and pads K - 1 - p.  mask_relu: dx holds relu(z) on entry and the result
// is exactly 0 where that is not > 0.
CXN_API int cxn_dwlk_bwd_data(const void *dy, long dys, const void *w, void *dx, long dxs, int N, int H, int W,
                              int C, int Cout, int groups, int KH, int KW, int stride, int pad_y, int pad_x,
                              int mask_relu, void *stream) {
  int Ho, Wo;
  if (!serves(N, H, W, C, Cout, groups, KH, KW, stride, pad_y, pad_x, Ho, Wo)) return -1;
  if (!operands_ok(dy, dys, dx, dxs, C) || (reinterpret_cast<uintptr_t>(w) & 1)) return -1;
  LArgs a;
  if (!make_args(a, N, Ho, Wo, H, W, C, dys, dxs, -(KH - 1 - pad_y), -(KW - 1 - pad_x))) return -1;
  return launch_stencil(true, KH, dy, w, nullptr, dx, a, mask_relu, stream);
}

// dw [C][KH][KW] += sum over pixels of dy x; db [C] (nullable) += sum of dy.  ws: fp32 workspace of
// ws_floats >= P C (K K + 1), P the slab count below (mirrored by ops.gemm.dwlk_wgrad_partials);
// -2 when it is smaller.
CXN_API int cxn_dwlk_bwd_weight(const void *x, long xs, const void *dy, long dys, float *dw, float *db, float *ws,
                                long ws_floats, int N, int H, int W, int C, int Cout, int groups, int KH, int KW,
                                int stride, int pad_y, int pad_x, void *stream) {
  int Ho, Wo;
  if (!serves(N, H, W, C, Cout, groups, KH, KW, stride, pad_y, pad_x, Ho, Wo)) return -1;
  if (!operands_ok(x, xs, dy, dys, C)) return -1;
  LArgs a;
  if (!make_args(a, N, H, W, Ho, Wo, C, xs, dys, -pad_y, -pad_x)) return -1;
  const int ny = channel_blocks(a);
  const long pmax = PMAX / ny > 1 ? PMAX / ny : 1;
  const long ipb = (static_cast<long>(a.items) + pmax - 1) / pmax;
  const int P = static_cast<int>((static_cast<long>(a.items) + ipb - 1) / ipb);
  const long slab = static_cast<long>(C) * (KH * KW + 1);
  if (!ws || static_cast<long>(P) * slab > ws_floats) return -2;
  const dim3 grid(static_cast<unsigned>(P), static_cast<unsigned>(ny));
  const bool sm = small_map(a.Hd, a.Wd);
#define CXN_LK_WG(T_)                                                                                               \
  CXN_LAUNCH((dwlk_wgrad_partial<T_>), grid, NT, 0, S_, (const bf16_t *)x, (const bf16_t *)dy, ws, a,                \
             static_cast<uint32_t>(ipb), C)
  if (KH == 7) {
    if (sm) CXN_LK_WG(Small<7>);
    else CXN_LK_WG(Big<7>);
  } else if (KH == 9) {
    if (sm) CXN_LK_WG(Small<9>);
    else CXN_LK_WG(Big<9>);
  } else {
    if (sm) CXN_LK_WG(Small<11>);
    else CXN_LK_WG(Big<11>);
  }
#undef CXN_LK_WG
  const int nw = C * KH * KW;
  CXN_LAUNCH((dwconv_wgrad_merge), (nw + C + MC - 1) / MC, NT, 0, S_, (const float *)ws, P, slab, dw, db, nw, C);
  RET;
}
