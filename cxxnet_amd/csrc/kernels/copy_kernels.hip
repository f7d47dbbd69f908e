// copies: element-wise sums, fan-out, channel slices and concatenation, padded copies and casts
// between the layers' buffers.  bf16 unless named otherwise; the 16-byte forms need every count
// and offset a multiple of 8 elements.
//
//   cxn_cast_f32_bf16                  y = bf16(x)
//   cxn_add_bf16, cxn_sum_bf16         y = a + b; y = s0 + .. + s3, optionally relu'-masked
//   cxn_fanout_bf16                    one source copied to up to 4 destinations
//   cxn_channel_copy, cxn_concat       channel slices of NHWC tensors, one slice or a whole concat
//   cxn_pad_rows, cxn_pad_interior     row-padded and zero-bordered copies
//   cxn_add_rows_f32                   dst rows += src rows of a wider fp32 buffer
//
// Return 0, a negative code for a shape they do not serve, or -3 when a launch failed.
#include "nn_shared.h"

namespace {
__global__ void cast_f32_bf16(const float *__restrict__ x, bf16_t *__restrict__ y, long n) {
  for (long i = grid_stride_start(); i < n; i += grid_stride()) y[i] = f2bf(x[i]);
}
__global__ void add_bf16(const bf16_t *a, const bf16_t *b, bf16_t *y, long n) {
  const long n8 = n / 8;
  if (blockIdx.x == 0 && threadIdx.x < n - n8 * 8) {
    const long i = n8 * 8 + threadIdx.x;
    y[i] = f2bf(bf2f(a[i]) + bf2f(b[i]));
  }
  for (long i = grid_stride_start(); i < n8; i += grid_stride()) {
    float x[8], z[8];
    unpack8(reinterpret_cast<const uint4 *>(a)[i], x);
    unpack8(reinterpret_cast<const uint4 *>(b)[i], z);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] += z[e];
    reinterpret_cast<uint4 *>(y)[i] = pack8(x);
  }
}
// split forward: one read of the source, up to 4 copies written (n8 16-byte vectors)
__global__ void fanout_bf16(const uint4 *__restrict__ src, uint4 *d0, uint4 *d1, uint4 *d2, uint4 *d3, int nd,
                            long n8) {
  for (long i = grid_stride_start(); i < n8; i += grid_stride()) {
    const uint4 v = src[i];
    d0[i] = v;
    if (nd > 1) d1[i] = v;
    if (nd > 2) d2[i] = v;
    if (nd > 3) d3[i] = v;
  }
}
// split backward: y = s0 + s1 (+ s2 + s3) in fp32, rounded once (y may alias s0)
// mask: y holds relu(z) on entry and the sum is kept only where y > 0 (relu') -- the backward
// of a split whose input is a zero-copy ch_concat of fused conv+relu branches
__global__ void sum_bf16(const uint4 *s0, const uint4 *s1, const uint4 *s2, const uint4 *s3, int ns, uint4 *y,
                         long n8, int mask) {
  for (long i = grid_stride_start(); i < n8; i += grid_stride()) {
    float a[8], b[8], z[8];
    if (mask) unpack8(y[i], z);
    unpack8(s0[i], a);
    unpack8(s1[i], b);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] += b[e];
    if (ns > 2) {
      unpack8(s2[i], b);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += b[e];
    }
    if (ns > 3) {
      unpack8(s3[i], b);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += b[e];
    }
    if (mask) {
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] = z[e] > 0.f ? a[e] : 0.f;
    }
    y[i] = pack8(a);
  }
}
}  // namespace

CXN_API int cxn_cast_f32_bf16(const float *x, void *y, long n, void *stream) {
  CXN_LAUNCH((cast_f32_bf16), nblocks(n), NT, 0, S_, x, (bf16_t *)y, n);
  RET;
}
CXN_API int cxn_add_bf16(const void *a, const void *b, void *y, long n, void *stream) {
  CXN_LAUNCH((add_bf16), nblocks(n / 8 + 1), NT, 0, S_, (const bf16_t *)a, (const bf16_t *)b, (bf16_t *)y, n);
  RET;
}
CXN_API int cxn_fanout_bf16(const void *src, void *d0, void *d1, void *d2, void *d3, int nd, long n, void *stream) {
  if (nd < 1 || nd > 4 || (n & 7) != 0) return -2;
  const long n8 = n / 8;
  CXN_LAUNCH((fanout_bf16), nblocks(n8), NT, 0, S_, (const uint4 *)src, (uint4 *)d0, (uint4 *)d1, (uint4 *)d2, (uint4 *)d3, nd,
                                          n8);
  RET;
}
CXN_API int cxn_sum_bf16(const void *s0, const void *s1, const void *s2, const void *s3, int ns, void *y, long n,
                         void *stream, int mask) {
  if (ns < 2 || ns > 4 || (n & 7) != 0) return -2;
  const long n8 = n / 8;
  CXN_LAUNCH((sum_bf16), nblocks(n8), NT, 0, S_, (const uint4 *)s0, (const uint4 *)s1, (const uint4 *)s2, (const uint4 *)s3, ns,
                                       (uint4 *)y, n8, mask);
  RET;
}

namespace {
// strided channel copy for ch_concat / slicing: dst[p][doff + c] = src[p][soff + c], c < Cc
// mode 0: copy; 1: accumulate (dst += src); 2: relu'-masked copy (dst holds relu(z): keep
// src where dst > 0) -- the backward of a ch_concat whose input came from a fused conv+relu
__global__ void channel_copy(const bf16_t *__restrict__ src, int Cs, int soff, bf16_t *__restrict__ dst, int Cd,
                             int doff, int Cc, long npix, int mode) {
  const long total = npix * Cc;
  for (long i = grid_stride_start(); i < total; i += grid_stride()) {
    const long p = i / Cc;
    const int c = i % Cc;
    const float v = bf2f(src[p * Cs + soff + c]);
    bf16_t *d = dst + p * Cd + doff + c;
    const float o = bf2f(*d);
    *d = f2bf(mode == 1 ? o + v : (mode == 2 && !(o > 0.f)) ? 0.f : v);
  }
}

// 8-channel (16-byte) form of channel_copy when every stride/offset/count is a multiple of 8
// (all GoogLeNet concat branches): one uint4 per lane, 32-bit index math (total8 < 2^31).
__global__ void channel_copy8(const uint4 *__restrict__ src, int Cs8, int soff8, uint4 *__restrict__ dst, int Cd8,
                              int doff8, int Cc8, uint32_t total8, int mode) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total8; i += gridDim.x * blockDim.x) {
    const uint32_t p = i / static_cast<uint32_t>(Cc8);
    const uint32_t c = i - p * static_cast<uint32_t>(Cc8);
    uint4 v = src[static_cast<size_t>(p) * Cs8 + soff8 + c];
    uint4 *d = dst + static_cast<size_t>(p) * Cd8 + doff8 + c;
    if (mode != 0) {
      float a[8], b[8];
      unpack8(v, a);
      unpack8(*d, b);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] = mode == 1 ? a[e] + b[e] : (b[e] > 0.f ? a[e] : 0.f);
      v = pack8(a);
    }
    *d = v;
  }
}
}  // namespace

CXN_API int cxn_channel_copy(const void *src, int Cs, int soff, void *dst, int Cd, int doff, int Cc, long npix,
                             int accumulate, void *stream) {
  const long total8 = npix * (Cc / 8);
  if (((Cs | soff | Cd | doff | Cc) & 7) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0 &&
      total8 > 0 && total8 < (1L << 31)) {
    CXN_LAUNCH((channel_copy8), nblocks(total8), NT, 0, S_, (const uint4 *)src, Cs / 8, soff / 8, (uint4 *)dst, Cd / 8, doff / 8,
                                                  Cc / 8, static_cast<uint32_t>(total8), accumulate);
    RET;
  }
  CXN_LAUNCH((channel_copy), nblocks(npix * Cc), NT, 0, S_, (const bf16_t *)src, Cs, soff, (bf16_t *)dst, Cd, doff, Cc, npix,
                                                  accumulate);
  RET;
}

namespace {
// Channel concat of up to 4 NHWC inputs in ONE launch (every channel count a multiple of 8).
// Forward: out[p][off_k + c] = in_k[p][c].  Backward (bwd = 1): in_k[p][c] = out[p][off_k + c],
// masked by relu'(old in_k) for inputs produced by a fused conv+relu (mask bit k).
struct ConcatArgs {
  uint4 *in[4];
  int c8[4];    // channels / 8 per input
  int off8[4];  // channel offset / 8 in the output
};
__global__ void concat8(ConcatArgs a, int n, uint4 *__restrict__ out, int Ct8, uint32_t total8, int bwd, int mask) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total8; i += gridDim.x * blockDim.x) {
    const uint32_t p = i / static_cast<uint32_t>(Ct8);
    const int c = static_cast<int>(i - p * static_cast<uint32_t>(Ct8));
    int k = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q)
      if (q < n && c >= a.off8[q]) k = q;
    uint4 *src_in = a.in[k] + static_cast<size_t>(p) * a.c8[k] + (c - a.off8[k]);
    if (!bwd) {
      out[i] = *src_in;
    } else {
      uint4 v = out[i];
      if ((mask >> k) & 1) {
        float g[8], x[8];
        unpack8(v, g);
        unpack8(*src_in, x);
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = x[e] > 0.f ? g[e] : 0.f;
        v = pack8(g);
      }
      *src_in = v;
    }
  }
}
}  // namespace

// ins[k] (NHWC, cs[k] channels, k < n <= 4) <-> out (Ct channels), npix pixels; bwd: out -> ins
CXN_API int cxn_concat(void *const *ins, const int *cs, int n, void *out, int Ct, long npix, int bwd, int mask,
                       void *stream) {
  if (n < 1 || n > 4 || Ct % 8) return -1;
  ConcatArgs a{};
  int off = 0;
  for (int k = 0; k < n; ++k) {
    if (cs[k] % 8) return -1;
    a.in[k] = static_cast<uint4 *>(ins[k]);
    a.c8[k] = cs[k] / 8;
    a.off8[k] = off / 8;
    off += cs[k];
  }
  if (off != Ct) return -1;
  const long total8 = npix * (Ct / 8);
  if (total8 >= (1L << 32)) return -1;
  CXN_LAUNCH((concat8), nblocks(total8), NT, 0, S_, a, n, static_cast<uint4 *>(out), Ct / 8, static_cast<uint32_t>(total8), bwd,
                                          mask);
  RET;
}

namespace {
// dst[r][0:L] = src[r][0:L], dst[r][L:Lp] = 0 (row-padded copy, e.g. conv1 weights for the
// row-gather GEMM: [Cout][KH][KW*C] -> [Cout][KH][roundup(KW*C, 8)])
__global__ void pad_rows(const bf16_t *__restrict__ src, bf16_t *__restrict__ dst, long rows, int L, int Lp) {
  const long total = rows * Lp;
  for (long i = grid_stride_start(); i < total; i += grid_stride()) {
    const long r = i / Lp;
    const int c = static_cast<int>(i - r * Lp);
    dst[i] = c < L ? src[r * L + c] : static_cast<bf16_t>(0);
  }
}

// Interior of a zero-bordered NHWC copy: dst[n][h + py][w + px][:] = src[n][h][w][:] in units of
// U bytes per pixel-chunk (the pre-pad conv path's input copy; the border stays as written once)
template <typename U>
__global__ void pad_interior(const U *__restrict__ src, U *__restrict__ dst, long npix, int H, int W, int H2, int W2,
                             int py, int px, int cu) {
  const long total = npix * cu;
  for (long i = grid_stride_start(); i < total; i += grid_stride()) {
    const long p = i / cu;
    const int c = static_cast<int>(i - p * cu);
    const long n = p / (static_cast<long>(H) * W);
    const int r = static_cast<int>(p - n * H * W);
    const int h = r / W, w = r - h * W;
    dst[((n * H2 + h + py) * W2 + w + px) * cu + c] = src[i];
  }
}

// dst[r][0:L] += src[r][0:L] (fp32; src rows of Ls >= L elements): the row-padded weight-grad
// buffer of the conv1 row-run path added into the layer's gradient
__global__ void add_rows_f32(const float *__restrict__ src, float *__restrict__ dst, long rows, int L, int Ls) {
  const long total = rows * L;
  for (long i = grid_stride_start(); i < total; i += grid_stride()) {
    const long r = i / L;
    dst[i] += src[r * Ls + (i - r * L)];
  }
}
}  // namespace

CXN_API int cxn_pad_rows(const void *src, void *dst, long rows, int L, int Lp, void *stream) {
  CXN_LAUNCH((pad_rows), nblocks(rows * Lp), NT, 0, S_, (const bf16_t *)src, (bf16_t *)dst, rows, L, Lp);
  RET;
}
CXN_API int cxn_pad_interior(const void *src, void *dst, int N, int H, int W, int C, int H2, int W2, int py, int px,
                             void *stream) {
  const long npix = static_cast<long>(N) * H * W;
  const int bytes = C * 2;
  if (bytes % 8 == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 7) == 0) {
    CXN_LAUNCH((pad_interior<uint2>), nblocks(npix * (bytes / 8)), NT, 0, S_, (const uint2 *)src, (uint2 *)dst, npix, H, W,
               H2, W2, py, px, bytes / 8);
  } else {
    CXN_LAUNCH((pad_interior<bf16_t>), nblocks(npix * C), NT, 0, S_, (const bf16_t *)src, (bf16_t *)dst, npix, H, W, H2,
               W2, py, px, C);
  }
  RET;
}
CXN_API int cxn_add_rows_f32(const float *src, float *dst, long rows, int L, int Ls, void *stream) {
  if (rows <= 0 || L <= 0) return 0;
  CXN_LAUNCH((add_rows_f32), nblocks(rows * L), NT, 0, S_, src, dst, rows, L, Ls);
  RET;
}
