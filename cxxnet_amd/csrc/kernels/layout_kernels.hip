// layout: what carries data into, out of and between the NHWC bf16 layout of the layer kernels.
//
//   cxn_nchw_f32_to_nhwc_bf16   NCHW fp32 -> NHWC bf16 input node (channel pad, row pad)
//   cxn_image_u8_to_nhwc_bf16   decoded uint8 image batch -> input node, the augmenter's arithmetic fused in
//   cxn_nhwc_bf16_to_nchw_f32   NHWC bf16 -> NCHW fp32
//   cxn_transpose               batched 2-D transpose (flatten into the reference's NCHW feature order)
//   cxn_conv_weight_flip(_multi) conv weights transformed for the data gradient, one or every layer per launch
//
// Every entry point takes its stream last and returns 0, -2 for a shape it does not serve, or -3
// when a launch failed.
#include "nn_shared.h"

namespace {
// x: NCHW fp32 [N][C][H][W] -> y: NHWC bf16 [N][H][Wp][Cp] (channels >= C zero-filled; columns
// >= W of a row-padded node are left as they are)
__global__ void nchw_f32_to_nhwc_bf16(const float *__restrict__ x, bf16_t *__restrict__ y, int N, int C, int H,
                                      int W, int Cp, int Wp, float scale) {
  const long total = static_cast<long>(N) * H * W;
  for (long pix = grid_stride_start(); pix < total; pix += grid_stride()) {
    const long n = pix / (static_cast<long>(H) * W);
    const long hw = pix - n * H * W;
    const float *src = x + n * C * H * W + hw;
    const long row = pix / W;
    bf16_t *dst = y + (row * Wp + (pix - row * W)) * Cp;
    if (Cp == 4) {
      float v[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = c < C ? src[static_cast<long>(c) * H * W] * scale : 0.f;
      *reinterpret_cast<uint2 *>(dst) = make_uint2(pack2(v[0], v[1]),
                                                   pack2(v[2], v[3]));
      continue;
    }
    for (int c = 0; c < Cp; ++c) dst[c] = c < C ? f2bf(src[static_cast<long>(c) * H * W] * scale) : 0;
  }
}
}  // namespace

// Wp: the node's physical row width (>= W; row-padded first-conv input, see image_u8c3_nhwc3p)
CXN_API int cxn_nchw_f32_to_nhwc_bf16(const float *x, void *y, int N, int C, int H, int W, int Cp, int Wp,
                                      float scale, void *stream) {
  if (Wp < W) return -2;
  CXN_LAUNCH((nchw_f32_to_nhwc_bf16), nblocks(static_cast<long>(N) * H * W), NT, 0, S_, x, (bf16_t *)y, N, C, H, W, Cp, Wp,
                                                                              scale);
  RET;
}

namespace {
// Decoded image batch -> NHWC bf16 input node, with the reference augmenter's
// arithmetic fused in (src/io/iter_augment_proc-inl.hpp:98-162).  The host has
// already cropped and mirrored the uint8 pixels (cheap row copies); mean
// subtraction, contrast, illumination, scale and the bf16/NHWC/channel-pad
// conversion run here so only uint8 crosses PCIe.
//   pix  u8 [B][h][w][C]          prm int [B][4] = {crop_y, crop_x, mirrored, 0}
//   cm   f32 [B][2] = {contrast, illumination}
//   mode 0: y = d*scale                      (no mean)
//        1: y = ((d - mean[c])*ct + il)*scale (mean_value)
//        2: mean image [C][Hm][Wm] of the uncropped size, read at the crop offset
//        3: mean image [C][h][w] of the crop size
__global__ void image_u8_to_nhwc_bf16(const uint8_t *__restrict__ pix, const int *__restrict__ prm,
                                      const float *__restrict__ cm, const float *__restrict__ mean, int B, int h,
                                      int w, int C, int Cp, int Wp, int Hm, int Wm, int mode, float scale,
                                      bf16_t *__restrict__ y) {
  // grid: x over blockIdx.x*NT + tid, one image row (b, r) per blockIdx.y: no per-pixel division
  const int row = blockIdx.y;
  const int b = row / h, r = row - b * h;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= w) return;
  const long p = static_cast<long>(row) * w + x;
  const uint8_t *src = pix + p * C;
  float ct = 1.f, il = 0.f;
  if (mode != 0) {
    ct = cm[2 * b];
    il = cm[2 * b + 1];
  }
  const int xs = (mode == 2 && prm[4 * b + 2]) ? (w - 1 - x) : x;
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    v[c] = 0.f;
    if (c < C && c < Cp) {
      const float d = static_cast<float>(src[c]);
      if (mode == 0) {
        v[c] = d * scale;
      } else {
        float m;
        if (mode == 1) m = mean[c];
        else if (mode == 2) m = mean[(static_cast<long>(c) * Hm + prm[4 * b] + r) * Wm + prm[4 * b + 1] + xs];
        else m = mean[(static_cast<long>(c) * h + r) * w + x];
        v[c] = ((d - m) * ct + il) * scale;
      }
    }
  }
  bf16_t *dst = y + (static_cast<long>(row) * Wp + x) * Cp;
  if (Cp == 4) {  // one 8-byte store per pixel
    *reinterpret_cast<uint2 *>(dst) = make_uint2(pack2(v[0], v[1]),
                                                 pack2(v[2], v[3]));
  } else {
    for (int c = 0; c < Cp; ++c) dst[c] = c < 8 ? f2bf(v[c]) : static_cast<bf16_t>(0);
  }
}

// Fast path of the above for the common case: C = 3, Cp = 4, mode 0/1, pixel count a
// multiple of 4.  Four pixels per thread: three aligned 4-byte loads, two 16-byte stores.
__global__ void image_u8c3_nhwc4(const uint32_t *__restrict__ pix, const float *__restrict__ cm,
                                 const float *__restrict__ mean, long quads, FastDiv fd_hw, int mode, float scale,
                                 uint4 *__restrict__ y) {
  for (long q = grid_stride_start(); q < quads; q += grid_stride()) {
    const uint32_t w0 = pix[3 * q], w1 = pix[3 * q + 1], w2 = pix[3 * q + 2];
    const uint32_t bytes[3] = {w0, w1, w2};
    float out[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t p = static_cast<uint32_t>(4 * q + k);
      float ct = 1.f, il = 0.f;
      if (mode == 1) {
        const uint32_t b = fdiv(p, fd_hw);
        ct = cm[2 * b];
        il = cm[2 * b + 1];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int byte = 3 * k + c;
        const float d = static_cast<float>((bytes[byte >> 2] >> (8 * (byte & 3))) & 0xffu);
        out[4 * k + c] = mode == 1 ? ((d - mean[c]) * ct + il) * scale : d * scale;
      }
      out[4 * k + 3] = 0.f;
    }
    y[2 * q] = pack8(out);
    y[2 * q + 1] = pack8(out + 8);
  }
}

// Fast path for the row-padded 3-channel node of a first conv on kernel-row runs
// (NeuralNet._pad_input_channels: AlexNet conv1 reads [B][h][Wp][3] with Wp % 4 == 0, so every
// image row and every 4-pixel group starts 8-byte aligned): one thread per 4 output pixels of a
// padded row, three 8-byte stores; the pad columns (x >= w) get zeros.  mode 0/1.  The 12 source
// bytes of a group start at any byte (rows of w*3 bytes): 4 aligned dword loads + alignbyte.
// Consecutive groups are consecutive 24-byte pieces of y (Wp % 4 == 0), so a full wave's output is
// one 1536-byte run: it goes through LDS and out as 16-byte stores (two per lane, the second on
// half the lanes) instead of three 8-byte stores at a 24-byte lane stride.
__global__ void __launch_bounds__(NT)
image_u8c3_nhwc3p(const uint32_t *__restrict__ pix, long ndw, const float *__restrict__ cm,
                  const float *__restrict__ mean, FastDiv fd_qpr, FastDiv fd_h, int w, int Wp,
                  int mode, float scale, uint32_t total, uint2 *__restrict__ y) {
  __shared__ __attribute__((aligned(16))) uint2 stage[NT * 3];
  const uint32_t q0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u);  // first group of this wave
  const uint32_t q = q0 + (threadIdx.x & 63u);
  if (q0 >= total) return;  // whole wave past the end
  const bool full = q0 + 64 <= total;
  if (!full && q >= total) return;  // (a partial wave stores directly below)
  const uint32_t row = fdiv(q, fd_qpr);
  const int x0 = static_cast<int>(q - row * fd_qpr.d) * 4;
  float ct = 1.f, il = 0.f;
  if (mode == 1) {
    const uint32_t b = fdiv(row, fd_h);
    ct = cm[2 * b];
    il = cm[2 * b + 1];
  }
  const long start = (static_cast<long>(row) * w + x0) * 3;
  const long d0 = start >> 2;
  const uint32_t sh = static_cast<uint32_t>(start & 3) * 8;
  uint32_t d[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) d[t] = pix[min(d0 + t, ndw - 1)];
  // bytes start .. start + 11 of the image batch as three dwords
  const uint32_t e[3] = {__builtin_amdgcn_alignbyte(d[1], d[0], sh >> 3), __builtin_amdgcn_alignbyte(d[2], d[1], sh >> 3),
                         __builtin_amdgcn_alignbyte(d[3], d[2], sh >> 3)};
  float out[12];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int byte = 3 * k + c;
      float v = 0.f;
      if (x0 + k < w) {
        const float dv = static_cast<float>((e[byte >> 2] >> (8 * (byte & 3))) & 0xffu);
        v = mode == 1 ? ((dv - mean[c]) * ct + il) * scale : dv * scale;
      }
      out[3 * k + c] = v;
    }
  if (!full) {
    uint2 *dst = y + (static_cast<long>(row) * Wp + x0) * 3 / 4;  // 4 pixels = 24 bytes = three uint2
#pragma unroll
    for (int t = 0; t < 3; ++t)
      dst[t] = make_uint2(pack2(out[4 * t], out[4 * t + 1]),
                          pack2(out[4 * t + 2], out[4 * t + 3]));
    return;
  }
  const int lane = threadIdx.x & 63;
  uint2 *const ws = stage + (threadIdx.x >> 6) * 192;  // this wave's 1536 bytes
#pragma unroll
  for (int t = 0; t < 3; ++t)
    ws[3 * lane + t] = make_uint2(pack2(out[4 * t], out[4 * t + 1]), pack2(out[4 * t + 2], out[4 * t + 3]));
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  // the wave's run starts at y + q0 * 3 uint2 (q0 % 64 == 0: 16-byte aligned when y is)
  uint4 *const dst = reinterpret_cast<uint4 *>(y + static_cast<long>(q0) * 3);
  const uint4 *const src = reinterpret_cast<const uint4 *>(ws);
  dst[lane] = src[lane];
  if (lane < 32) dst[64 + lane] = src[64 + lane];
}
}  // namespace

CXN_API int cxn_image_u8_to_nhwc_bf16(const void *pix, const int *prm, const float *cm, const float *mean, int B,
                                      int h, int w, int C, int Cp, int Wp, int Hm, int Wm, int mode, float scale,
                                      void *y, void *stream) {
  if (Cp < C || Wp < w || (mode != 0 && cm == nullptr) || (mode >= 1 && mean == nullptr) ||
      (mode == 2 && prm == nullptr))
    return -2;
  if (C > 8) return -2;
  const long npix = static_cast<long>(B) * h * w;
  const long nq = static_cast<long>(B) * h * (Wp / 4);
  if (C == 3 && Cp == 3 && mode <= 1 && Wp % 4 == 0 && reinterpret_cast<uintptr_t>(y) % 16 == 0 &&
      reinterpret_cast<uintptr_t>(pix) % 4 == 0 && npix * 3 >= 16 && nq < (1L << 31)) {
    CXN_LAUNCH((image_u8c3_nhwc3p), cdiv(nq, NT), NT, 0, S_, (const uint32_t *)pix, (npix * 3 + 3) / 4, cm, mean,
                                                    make_fastdiv(static_cast<uint32_t>(Wp / 4)),
                                                    make_fastdiv(static_cast<uint32_t>(h)), w, Wp, mode, scale,
                                                    static_cast<uint32_t>(nq), (uint2 *)y);
    RET;
  }
  if (C == 3 && Cp == 4 && Wp == w && mode <= 1 && npix % 4 == 0 && npix < (1L << 32) &&
      reinterpret_cast<uintptr_t>(pix) % 4 == 0) {
    CXN_LAUNCH((image_u8c3_nhwc4), nblocks(npix / 4), NT, 0, S_, (const uint32_t *)pix, cm, mean, npix / 4,
                                                        make_fastdiv(static_cast<uint32_t>(h * w)), mode, scale,
                                                        (uint4 *)y);
    RET;
  }
  dim3 grid(cdiv(w, NT), B * h);
  CXN_LAUNCH((image_u8_to_nhwc_bf16), grid, NT, 0, S_, (const uint8_t *)pix, prm, cm, mean, B, h, w, C, Cp, Wp, Hm, Wm, mode,
                                             scale, (bf16_t *)y);
  RET;
}

namespace {
// x: NHWC bf16 [N][H][Wp][Cp] -> y: NCHW fp32 [N][C][H][W]
__global__ void nhwc_bf16_to_nchw_f32(const bf16_t *__restrict__ x, float *__restrict__ y, int N, int C, int H,
                                      int W, int Cp, int Wp) {
  const long total = static_cast<long>(N) * C * H * W;
  for (long i = grid_stride_start(); i < total; i += grid_stride()) {
    const long w = i % W;
    long t = i / W;
    const long h = t % H;
    t /= H;
    const long c = t % C;
    const long n = t / C;
    y[i] = bf2f(x[((n * H + h) * Wp + w) * Cp + c]);
  }
}
}  // namespace

CXN_API int cxn_nhwc_bf16_to_nchw_f32(const void *x, float *y, int N, int C, int H, int W, int Cp, int Wp,
                                      void *stream) {
  CXN_LAUNCH((nhwc_bf16_to_nchw_f32), nblocks(static_cast<long>(N) * C * H * W), NT, 0, S_, (const bf16_t *)x, y, N, C, H, W, Cp,
                                                                                  Wp);
  RET;
}

namespace {
// Batched 2-D transpose x[b][R][Cc] -> y[b][Cc][R] (bf16), tiled through LDS.
// Flatten of an NHWC activation into the reference's NCHW feature order is
// transpose(R=HW, Cc=C); its gradient is transpose(R=C, Cc=HW).
__global__ void batched_transpose(const bf16_t *__restrict__ x, bf16_t *__restrict__ y, int R, int Cc) {
  __shared__ bf16_t tile[32][34];
  const long base = static_cast<long>(blockIdx.z) * R * Cc;
  const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: 32 x 8
  for (int r = ty; r < 32; r += 8)
    if (r0 + r < R && c0 + tx < Cc) tile[r][tx] = x[base + static_cast<long>(r0 + r) * Cc + c0 + tx];
  __syncthreads();
  for (int c = ty; c < 32; c += 8)
    if (c0 + c < Cc && r0 + tx < R) y[base + static_cast<long>(c0 + c) * R + r0 + tx] = tile[tx][c];
}

// Small per-item matrices (AlexNet's flatten: 36 x 256 and back): one block per item stages the
// whole matrix in LDS with 8-byte loads (rows padded by 2 elements: the transposed reads of 32
// consecutive rows fall on 32 different banks) and writes the transpose as 4-byte pairs of
// consecutive output elements.  The 32 x 32 tiled form moved 2-byte elements in 4096 blocks
// (7.8 us for 4.7 MB at batch 256).
__global__ void __launch_bounds__(256) batched_transpose_item(const bf16_t *__restrict__ x, bf16_t *__restrict__ y,
                                                                int R, int Cc) {
  extern __shared__ __attribute__((aligned(16))) uint16_t tl[];
  const int ld = Cc + 2;
  const long base = static_cast<long>(blockIdx.x) * R * Cc;
  const uint2 *xs = reinterpret_cast<const uint2 *>(x + base);
  const int nq = R * Cc / 4;
  for (int i = threadIdx.x; i < nq; i += blockDim.x) {
    const uint2 v = xs[i];
    const int e = 4 * i, r = e / Cc, c = e - r * Cc;
    uint32_t *d = reinterpret_cast<uint32_t *>(tl + r * ld + c);  // 4-byte aligned: ld and c are even
    d[0] = v.x;
    d[1] = v.y;
  }
  __syncthreads();
  uint32_t *ys = reinterpret_cast<uint32_t *>(y + base);
  const int np = R * Cc / 2;
  for (int i = threadIdx.x; i < np; i += blockDim.x) {
    const int o = 2 * i, c = o / R, r = o - c * R;  // output (c, r) and (c', r') of o + 1
    const int o1 = o + 1, c1 = o1 / R, r1 = o1 - c1 * R;
    ys[i] = static_cast<uint32_t>(tl[r * ld + c]) | (static_cast<uint32_t>(tl[r1 * ld + c1]) << 16);
  }
}
}  // namespace

CXN_API int cxn_transpose(const void *x, void *y, int B, int R, int Cc, void *stream) {
  const size_t lds = static_cast<size_t>(R) * (Cc + 2) * 2;
  if (Cc % 4 == 0 && R % 2 == 0 && lds <= 48 * 1024 && B >= 64 && reinterpret_cast<uintptr_t>(x) % 8 == 0 &&
      reinterpret_cast<uintptr_t>(y) % 4 == 0) {
    CXN_LAUNCH((batched_transpose_item), B, 256, lds, S_, (const bf16_t *)x, (bf16_t *)y, R, Cc);
    RET;
  }
  dim3 grid(cdiv(R, 32), cdiv(Cc, 32), B);
  CXN_LAUNCH((batched_transpose), grid, NT, 0, S_, (const bf16_t *)x, (bf16_t *)y, R, Cc);
  RET;
}

namespace {
// Conv weight transform for data-grad: W[g][co][kh][kw][ci] -> Wt[g][ci][KH-1-kh][KW-1-kw][co]
__global__ void conv_weight_flip(const bf16_t *__restrict__ w, bf16_t *__restrict__ wt, int G, int Co, int KH,
                                 int KW, int Ci) {
  const long total = static_cast<long>(G) * Co * KH * KW * Ci;
  for (long i = grid_stride_start(); i < total; i += grid_stride()) {
    long t = i;
    const int ci = t % Ci; t /= Ci;
    const int kw = t % KW; t /= KW;
    const int kh = t % KH; t /= KH;
    const int co = t % Co;
    const int g = t / Co;
    const long o = ((((static_cast<long>(g) * Ci + ci) * KH + (KH - 1 - kh)) * KW + (KW - 1 - kw)) * Co) + co;
    wt[o] = w[i];
  }
}
}  // namespace

CXN_API int cxn_conv_weight_flip(const void *w, void *wt, int G, int Co, int KH, int KW, int Ci, void *stream) {
  CXN_LAUNCH((conv_weight_flip), nblocks(static_cast<long>(G) * Co * KH * KW * Ci), NT, 0, S_, (const bf16_t *)w, (bf16_t *)wt,
                                                                                     G, Co, KH, KW, Ci);
  RET;
}

namespace {
// Every conv layer's flipped weights of a backward pass in one launch (flat grid, blocks split over
// segments by size; 32-bit index math).  GoogLeNet flipped 56 weight tensors one launch each
// (≈5.7 us apiece, 64-bit divisions per element): 0.3 ms of a 6.8 ms step.
constexpr int FLIP_MAXSEG = 64;
struct FlipSeg {
  const bf16_t *w;
  bf16_t *wt;
  int Co, KH, KW, Ci, total;
};
struct FlipTable {
  FlipSeg s[FLIP_MAXSEG];
  int b0[FLIP_MAXSEG];
  int n;
};
// One block = one 64 x 64 (co, ci) tile of one (group, tap): read as 64 rows of contiguous ci,
// written as 64 rows of contiguous co through an LDS transpose.  (One element per thread with the
// output strided by Co ran at 0.6 TB/s -- 96 us per VGG-16 step.)
__global__ void conv_weight_flip_multi(FlipTable tab) {
  const int bx = blockIdx.x;
  int si = 0;
  for (int i = 1; i < tab.n; ++i)
    if (tab.b0[i] <= bx) si = i;
  const FlipSeg sg = tab.s[si];
  const int tco = (sg.Co + 63) / 64, tci = (sg.Ci + 63) / 64;
  int t = bx - tab.b0[si];
  const int ci0 = (t % tci) * 64; t /= tci;
  const int co0 = (t % tco) * 64; t /= tco;
  const int kw = t % sg.KW; t /= sg.KW;
  const int kh = t % sg.KH;
  const int g = t / sg.KH;
  __shared__ uint32_t tile[64][65];
  const int col = threadIdx.x & 63;
  const unsigned short *w = reinterpret_cast<const unsigned short *>(sg.w);
  unsigned short *wt = reinterpret_cast<unsigned short *>(sg.wt);
  if ((sg.Co & 7) == 0 && (sg.Ci & 7) == 0) {
    // 16-byte accesses: lane (r8, c8) moves 8 consecutive channels of one row (the 2-byte form
    // below issued 8x the memory instructions: AlexNet's 7.5 MB of conv weights took 12 us)
    unsigned short *tl = reinterpret_cast<unsigned short *>(tile);  // [64][130] bf16 (pitch 65 words)
    const int c8 = (threadIdx.x & 7) * 8, r8 = threadIdx.x >> 3;
    for (int r = r8; r < 64; r += NT / 8) {
      const int co = co0 + r, ci = ci0 + c8;
      if (co < sg.Co && ci < sg.Ci) {
        const uint4 v = *reinterpret_cast<const uint4 *>(w + (((g * sg.Co + co) * sg.KH + kh) * sg.KW + kw) * sg.Ci + ci);
        const unsigned short *e = reinterpret_cast<const unsigned short *>(&v);
#pragma unroll
        for (int k = 0; k < 8; ++k) tl[r * 130 + c8 + k] = e[k];
      }
    }
    __syncthreads();
    for (int r = r8; r < 64; r += NT / 8) {  // r = ci within the tile, c8 = first co
      const int ci = ci0 + r, co = co0 + c8;
      if (co < sg.Co && ci < sg.Ci) {
        uint4 v;
        unsigned short *e = reinterpret_cast<unsigned short *>(&v);
#pragma unroll
        for (int k = 0; k < 8; ++k) e[k] = tl[(c8 + k) * 130 + r];
        *reinterpret_cast<uint4 *>(wt + (((g * sg.Ci + ci) * sg.KH + (sg.KH - 1 - kh)) * sg.KW + (sg.KW - 1 - kw)) * sg.Co +
                                   co) = v;
      }
    }
    return;
  }
  for (int r = threadIdx.x >> 6; r < 64; r += NT / 64) {
    const int co = co0 + r, ci = ci0 + col;
    if (co < sg.Co && ci < sg.Ci) tile[r][col] = w[(((g * sg.Co + co) * sg.KH + kh) * sg.KW + kw) * sg.Ci + ci];
  }
  __syncthreads();
  for (int r = threadIdx.x >> 6; r < 64; r += NT / 64) {
    const int ci = ci0 + r, co = co0 + col;
    if (co < sg.Co && ci < sg.Ci)
      wt[(((g * sg.Ci + ci) * sg.KH + (sg.KH - 1 - kh)) * sg.KW + (sg.KW - 1 - kw)) * sg.Co + co] =
          static_cast<unsigned short>(tile[col][r]);
  }
}
}  // namespace

// ws / wts: n weight tensors [G][Co][KH][KW][Ci] -> [G][Ci][KH'][KW'][Co] (taps reversed);
// dims: 5 ints per tensor (G, Co, KH, KW, Ci)
CXN_API int cxn_conv_weight_flip_multi(const void *const *ws, void *const *wts, const int *dims, int n, void *stream) {
  for (int base = 0; base < n; base += FLIP_MAXSEG) {
    FlipTable tab;
    const int cnt = n - base < FLIP_MAXSEG ? n - base : FLIP_MAXSEG;
    int nblk = 0;
    tab.n = cnt;
    for (int i = 0; i < cnt; ++i) {
      const int *d = dims + 5 * (base + i);
      const long total = static_cast<long>(d[0]) * d[1] * d[2] * d[3] * d[4];
      if (total >= (1L << 31)) return -2;
      tab.s[i] = FlipSeg{static_cast<const bf16_t *>(ws[base + i]), static_cast<bf16_t *>(wts[base + i]), d[1], d[2],
                         d[3], d[4], static_cast<int>(total)};
      tab.b0[i] = nblk;
      nblk += d[0] * d[2] * d[3] * cdiv(d[1], 64) * cdiv(d[4], 64);  // 64 x 64 (co, ci) tiles per (g, tap)
    }
    if (nblk) CXN_LAUNCH((conv_weight_flip_multi), nblk, NT, 0, S_, tab);
  }
  RET;
}
