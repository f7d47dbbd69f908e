// pooling: max / sum / avg forward and gather-form backward on NHWC bf16 (reference
// src/layer/pooling_layer-inl.hpp:42-111).
//
//   cxn_pool_fwd           y (and, in max mode, the offset byte of each window's first maximum)
//   cxn_pool_bwd           dx from (dy, offsets); with db also the bias gradient of the conv in front
//   cxn_pool_bwd_tie_all   max-unpool with the reference's tie semantics (pool_tie = all)
//
// Each launcher picks the most specific kernel that serves the shape: the stride-1 3x3 strips
// (_s1k3), the stride-2 3x3 cells (_s2k3, backward), the fixed-window one-element-per-thread
// forms (_rows; C % 8 == 0 and < 2^31 items), else the grid-stride forms.  They return 0, -2 for
// a shape or workspace they cannot serve, or -3 when a launch failed.
#include "nn_shared.h"

namespace {
// mode: 0 max, 1 sum, 2 avg.  relu bit 0: apply relu before max (relu_max_pooling);
// relu bit 1 (max mode, KH*KW < 128): set bit 7 of the recorded offset when the window
// maximum is <= 0, so the backward can apply relu' of the argmax element without
// re-reading the (large) input: relu'(x[argmax]) = (max > 0).
// Output size follows the reference ceil rule: min(Hp - k + s - 1, Hp - 1) / s + 1, Hp = H + 2 pad.
// Max mode records, per output, the window offset (kh*KW + kw, uint8) of the FIRST maximum.
template <int VEC>
__global__ void pool_fwd(const bf16_t *__restrict__ x, bf16_t *__restrict__ y, uint8_t *__restrict__ arg, int N,
                         int H, int W, int C, int Ho, int Wo, int KH, int KW, int S, int P, int mode, int relu) {
  const int CV = C / VEC;
  const long total = static_cast<long>(N) * Ho * Wo * CV;
  const float inv = 1.0f / (KH * KW);
  for (long idx = grid_stride_start(); idx < total; idx += grid_stride()) {
    const int cv = idx % CV;
    long t = idx / CV;
    const int wo = t % Wo; t /= Wo;
    const int ho = t % Ho;
    const int n = t / Ho;
    const int hs = ho * S - P, ws = wo * S - P;
    const int he = min(hs + KH, H), we = min(ws + KW, W);
    float acc[VEC];
    uint32_t am[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      acc[e] = mode == 0 ? -INFINITY : 0.f;
      am[e] = 0;
    }
    for (int h = max(hs, 0); h < he; ++h)
      for (int w = max(ws, 0); w < we; ++w) {
        const bf16_t *p = x + ((static_cast<long>(n) * H + h) * W + w) * C + cv * VEC;
        const uint32_t off = static_cast<uint32_t>((h - hs) * KW + (w - ws));
        float v[VEC];
        if constexpr (VEC == 8) unpack8(*reinterpret_cast<const uint4 *>(p), v);
        else v[0] = bf2f(*p);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float a = (relu & 1) ? fmaxf(v[e], 0.f) : v[e];
          if (mode == 0) {
            if (a > acc[e]) {
              acc[e] = a;
              am[e] = off;
            }
          } else {
            acc[e] += a;
          }
        }
      }
    if (mode == 2)
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] *= inv;
    if (mode == 0 && (relu & 2))
#pragma unroll
      for (int e = 0; e < VEC; ++e) am[e] |= acc[e] > 0.f ? 0u : 0x80u;
    if constexpr (VEC == 8) {
      *reinterpret_cast<uint4 *>(y + idx * VEC) = pack8(acc);
      if (arg)
        *reinterpret_cast<uint2 *>(arg + idx * VEC) =
            make_uint2(am[0] | am[1] << 8 | am[2] << 16 | am[3] << 24, am[4] | am[5] << 8 | am[6] << 16 | am[7] << 24);
    } else {
      y[idx] = f2bf(acc[0]);
      if (arg) arg[idx] = static_cast<uint8_t>(am[0]);
    }
  }
}

// One-element-per-thread forms of pool_fwd / pool_bwd for C % 8 == 0 and < 2^32
// elements: the index split is three 32-bit fast divisions (the grid-stride forms above
// spend most of their issue slots on 64-bit divisions).  Same semantics, including the
// relu' bit.
// SS / KS > 0: stride / square kernel fixed at compile time (3x3/2, 3x3/1, 2x2/2 -- every
// pooling of the model zoo): constant divisions and fully unrolled windows.
// NN (max mode, fixed window, relu & 4 and not relu & 1): the input is a relu output (>= 0), so
// bf16 bits order as unsigned integers and the first max is one v_max_u32 per element over keys
// (bits << 16 | 15 - tap; see pool_lrn_fwd) instead of unpack + compare + two selects.
__device__ __forceinline__ uint32_t nn_key_lo(uint32_t w, uint32_t t) { return ((w << 16) & 0x7fff0000u) | t; }
__device__ __forceinline__ uint32_t nn_key_hi(uint32_t w, uint32_t t) { return (w & 0x7fff0000u) | t; }
template <int SS, int KS, bool NN = false>
__global__ void pool_fwd_rows(const bf16_t *__restrict__ x, bf16_t *__restrict__ y, uint8_t *__restrict__ arg, int H,
                              int W, int C, int Ho, int Wo, int KHr, int KWr, int Sr, int P, int mode, int relu,
                              FastDiv fd_cv, FastDiv fd_row, FastDiv fd_h, uint32_t total) {
  const int S = SS > 0 ? SS : Sr, KH = KS > 0 ? KS : KHr, KW = KS > 0 ? KS : KWr;
  const int CV = C / 8;
  // XCD-aware: consecutive logical blocks (overlapping windows read the same input rows)
  // run on one XCD and share its L2 instead of re-fetching the overlap per XCD
  const uint32_t idx = xcd_remap(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int row = static_cast<int>(fdiv(idx, fd_row));           // n * Ho + ho
  const int e = static_cast<int>(idx) - row * (Wo * CV);
  const int n = static_cast<int>(fdiv(static_cast<uint32_t>(row), fd_h)), ho = row - n * Ho;
  const int wo = static_cast<int>(fdiv(static_cast<uint32_t>(e), fd_cv));
  const int cv = e - wo * CV;
  const int hs = ho * S - P, ws = wo * S - P;
  const int he = min(hs + KH, H), we = min(ws + KW, W);
  float acc[8];
  uint32_t am[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    acc[q] = mode == 0 ? -INFINITY : 0.f;
    am[q] = 0;
  }
  const bf16_t *xb = x + static_cast<long>(n) * H * W * C + cv * 8;
  auto take = [&](const uint4 raw, uint32_t off) {
    float v[8];
    unpack8(raw, v);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float a = (relu & 1) ? fmaxf(v[q], 0.f) : v[q];
      if (mode == 0) {
        if (a > acc[q]) {
          acc[q] = a;
          am[q] = off;
        }
      } else {
        acc[q] += a;
      }
    }
  };
  if constexpr (KS > 0) {
    // fixed window: all KS*KS loads issued back to back (clamped addresses, edge taps
    // masked), then reduced in the same h-major order as the generic loop (first max wins)
    uint4 raw[KS * KS];
#pragma unroll
    for (int kh = 0; kh < KS; ++kh)
#pragma unroll
      for (int kw = 0; kw < KS; ++kw) {
        const int h = min(max(hs + kh, 0), H - 1), w = min(max(ws + kw, 0), W - 1);
        raw[kh * KS + kw] = *reinterpret_cast<const uint4 *>(xb + (static_cast<long>(h) * W + w) * C);
      }
    if constexpr (NN) {
      uint32_t best[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) best[q] = 0u;
#pragma unroll
      for (int kh = 0; kh < KS; ++kh)
#pragma unroll
        for (int kw = 0; kw < KS; ++kw)
          if (hs + kh >= 0 && hs + kh < he && ws + kw >= 0 && ws + kw < we) {
            const uint32_t t = 15u - static_cast<uint32_t>(kh * KS + kw);
            const uint4 r = raw[kh * KS + kw];
            const uint32_t wd[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              best[2 * q] = max(best[2 * q], nn_key_lo(wd[q], t));
              best[2 * q + 1] = max(best[2 * q + 1], nn_key_hi(wd[q], t));
            }
          }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        acc[q] = __uint_as_float(best[q] & 0x7fff0000u);
        am[q] = 15u - (best[q] & 15u);
      }
    } else {
#pragma unroll
      for (int kh = 0; kh < KS; ++kh)
#pragma unroll
        for (int kw = 0; kw < KS; ++kw)
          if (hs + kh >= 0 && hs + kh < he && ws + kw >= 0 && ws + kw < we)
            take(raw[kh * KS + kw], static_cast<uint32_t>(kh * KW + kw));
    }
  } else {
    for (int h = max(hs, 0); h < he; ++h)
      for (int w = max(ws, 0); w < we; ++w)
        take(*reinterpret_cast<const uint4 *>(xb + (static_cast<long>(h) * W + w) * C),
             static_cast<uint32_t>((h - hs) * KW + (w - ws)));
  }
  if (mode == 2) {
    const float inv = 1.0f / (KH * KW);
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] *= inv;
  }
  if (mode == 0 && (relu & 2))
#pragma unroll
    for (int q = 0; q < 8; ++q) am[q] |= acc[q] > 0.f ? 0u : 0x80u;
  const long o = (static_cast<long>(row) * Wo + wo) * C + cv * 8;
  *reinterpret_cast<uint4 *>(y + o) = pack8(acc);
  if (arg)
    *reinterpret_cast<uint2 *>(arg + o) =
        make_uint2(am[0] | am[1] << 8 | am[2] << 16 | am[3] << 24, am[4] | am[5] << 8 | am[6] << 16 | am[7] << 24);
}

// Stride-1 3x3 max pooling (GoogLeNet's inception pool branches) on strips of R output rows per
// thread: each input row of the strip is read once as a 3-tap row maximum (value + kw), and every
// output row takes the row maxima of its three input rows -- (R + 2) * 3 loads per R outputs
// instead of 9 per output.  Same first-max order (kh, then kw) and relu flags as pool_fwd_rows.
// NN: integer keys as pool_fwd_rows (row key bits << 16 | 3 - kw; the output key adds 12 - 3 kh,
// giving bits << 16 | 15 - (3 kh + kw)).
template <int R, bool NN = false>
__global__ void pool_fwd_s1k3(const bf16_t *__restrict__ x, bf16_t *__restrict__ y, uint8_t *__restrict__ arg,
                              int H, int W, int C, int Ho, int Wo, int P, int relu, FastDiv fd_cv, FastDiv fd_row,
                              FastDiv fd_hs, uint32_t total) {
  const int CV = C / 8, HS = (Ho + R - 1) / R;
  const uint32_t idx = xcd_remap(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int row = static_cast<int>(fdiv(idx, fd_row));  // n * HS + strip
  const int e = static_cast<int>(idx) - row * (Wo * CV);
  const int n = static_cast<int>(fdiv(static_cast<uint32_t>(row), fd_hs)), st = row - n * HS;
  const int wo = static_cast<int>(fdiv(static_cast<uint32_t>(e), fd_cv));
  const int cv = e - wo * CV;
  const int ho0 = st * R, h0 = ho0 - P, ws = wo - P;
  const bf16_t *xb = x + static_cast<long>(n) * H * W * C + cv * 8;
  float acc[R][8];
  uint32_t am[R][8];
#pragma unroll
  for (int o = 0; o < R; ++o)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      acc[o][q] = -INFINITY;
      am[o][q] = 0;
    }
  if constexpr (NN) {
    uint32_t best[R][8];
#pragma unroll
    for (int o = 0; o < R; ++o)
#pragma unroll
      for (int q = 0; q < 8; ++q) best[o][q] = 0u;
#pragma unroll
    for (int r = 0; r < R + 2; ++r) {
      const int h = h0 + r;
      if (h < 0 || h >= H) continue;
      uint4 raw[3];
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int w = min(max(ws + kw, 0), W - 1);
        raw[kw] = *reinterpret_cast<const uint4 *>(xb + (static_cast<long>(h) * W + w) * C);
      }
      uint32_t rk[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) rk[q] = 0u;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        if (ws + kw < 0 || ws + kw >= W) continue;
        const uint32_t t = 3u - static_cast<uint32_t>(kw);
        const uint32_t wd[4] = {raw[kw].x, raw[kw].y, raw[kw].z, raw[kw].w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          rk[2 * q] = max(rk[2 * q], nn_key_lo(wd[q], t));
          rk[2 * q + 1] = max(rk[2 * q + 1], nn_key_hi(wd[q], t));
        }
      }
#pragma unroll
      for (int o = 0; o < R; ++o) {
        const int kh = r - o;
        if (kh < 0 || kh > 2) continue;
#pragma unroll
        for (int q = 0; q < 8; ++q)  // (every row has a valid tap: rk >= 1)
          best[o][q] = max(best[o][q], rk[q] + static_cast<uint32_t>(12 - 3 * kh));
      }
    }
#pragma unroll
    for (int o = 0; o < R; ++o)
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        acc[o][q] = __uint_as_float(best[o][q] & 0x7fff0000u);
        am[o][q] = 15u - (best[o][q] & 15u);
      }
  } else {
#pragma unroll
  for (int r = 0; r < R + 2; ++r) {
    const int h = h0 + r;
    if (h < 0 || h >= H) continue;
    uint4 raw[3];
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int w = min(max(ws + kw, 0), W - 1);
      raw[kw] = *reinterpret_cast<const uint4 *>(xb + (static_cast<long>(h) * W + w) * C);
    }
    float hm[8];
    uint32_t hk[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      hm[q] = -INFINITY;
      hk[q] = 0;
    }
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      if (ws + kw < 0 || ws + kw >= W) continue;
      float v[8];
      unpack8(raw[kw], v);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float a = (relu & 1) ? fmaxf(v[q], 0.f) : v[q];
        if (a > hm[q]) {
          hm[q] = a;
          hk[q] = kw;
        }
      }
    }
    // output rows o of the strip whose window holds input row r at kh = r - o
#pragma unroll
    for (int o = 0; o < R; ++o) {
      const int kh = r - o;
      if (kh < 0 || kh > 2) continue;
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (hm[q] > acc[o][q]) {
          acc[o][q] = hm[q];
          am[o][q] = static_cast<uint32_t>(kh * 3) + hk[q];
        }
    }
  }
  }
#pragma unroll
  for (int o = 0; o < R; ++o) {
    const int ho = ho0 + o;
    if (ho >= Ho) break;
    if (relu & 2)
#pragma unroll
      for (int q = 0; q < 8; ++q) am[o][q] |= acc[o][q] > 0.f ? 0u : 0x80u;
    const long off = ((static_cast<long>(n) * Ho + ho) * Wo + wo) * C + cv * 8;
    *reinterpret_cast<uint4 *>(y + off) = pack8(acc[o]);
    if (arg)
      *reinterpret_cast<uint2 *>(arg + off) =
          make_uint2(am[o][0] | am[o][1] << 8 | am[o][2] << 16 | am[o][3] << 24,
                     am[o][4] | am[o][5] << 8 | am[o][6] << 16 | am[o][7] << 24);
  }
}
}  // namespace

// stride-1 3x3 max pooling on row strips (pool_fwd_s1k3 / pool_bwd_s1k3); CXXNET_POOL_STRIPS=0 keeps
// the one-output-per-thread kernels (A/B)
static const int pool_strips = [] {
  const char *e = getenv("CXXNET_POOL_STRIPS");
  return (e && e[0] == '0') ? 0 : 1;
}();

CXN_API int cxn_pool_fwd(const void *x, void *y, void *arg, int N, int H, int W, int C, int Ho, int Wo, int KH, int KW, int S,
                         int P, int mode, int relu, void *stream) {
  if (C % 8 == 0) {
    const long total = static_cast<long>(N) * Ho * Wo * (C / 8);
    if (total >= (1L << 31)) return -2;  // fdiv (mulhi + n) stays exact below 2^31
    // relu & 4: the input is a relu output (>= 0): integer-key max (NN forms)
    const bool nn = mode == 0 && (relu & 4) != 0 && (relu & 1) == 0;
#define CXN_POOL_FWD_T(SSV, KSV, NNV)                                                                        \
  CXN_LAUNCH((pool_fwd_rows<SSV, KSV, NNV>), cdiv(total, NT), NT, 0, S_,                                     \
      (const bf16_t *)x, (bf16_t *)y, (uint8_t *)arg, H, W, C, Ho, Wo, KH, KW, S, P, mode, relu,             \
      make_fastdiv(static_cast<uint32_t>(C / 8)), make_fastdiv(static_cast<uint32_t>(Wo * (C / 8))),        \
      make_fastdiv(static_cast<uint32_t>(Ho)), static_cast<uint32_t>(total))
#define CXN_POOL_FWD(SSV, KSV) with_flag(nn, [&](auto nnv) { CXN_POOL_FWD_T(SSV, KSV, decltype(nnv)::value); })
    const int sq = KH == KW ? KH : 0;
    if (S == 1 && sq == 3 && mode == 0 && P <= 2 && pool_strips) {
      constexpr int R = 4;
      const int HS = (Ho + R - 1) / R;
      const long tot = static_cast<long>(N) * HS * Wo * (C / 8);
      with_flag(nn, [&](auto nnv) {
        CXN_LAUNCH((pool_fwd_s1k3<R, decltype(nnv)::value>), cdiv(tot, NT), NT, 0, S_, (const bf16_t *)x, (bf16_t *)y,
                   (uint8_t *)arg, H, W, C, Ho, Wo, P, relu, make_fastdiv(static_cast<uint32_t>(C / 8)),
                   make_fastdiv(static_cast<uint32_t>(Wo * (C / 8))), make_fastdiv(static_cast<uint32_t>(HS)),
                   static_cast<uint32_t>(tot));
      });
    } else if (S == 2 && sq == 3) CXN_POOL_FWD(2, 3);
    else if (S == 1 && sq == 3) CXN_POOL_FWD(1, 3);
    else if (S == 2 && sq == 2) CXN_POOL_FWD(2, 2);
    else CXN_POOL_FWD_T(0, 0, false);
#undef CXN_POOL_FWD
#undef CXN_POOL_FWD_T
  } else {
    CXN_LAUNCH((pool_fwd<1>), nblocks(static_cast<long>(N) * Ho * Wo * C), NT, 0, S_, 
        (const bf16_t *)x, (bf16_t *)y, (uint8_t *)arg, N, H, W, C, Ho, Wo, KH, KW, S, P, mode, relu);
  }
  RET;
}

namespace {
// Gather-form backward: each input element sums the gradients of the windows that contain
// it.  Max: the window's recorded first-maximum position receives the gradient (the
// reference compares values, src/layer/pooling_layer-inl.hpp:55-86, which with bf16
// activations would hand duplicates to rounding ties).  relu 1: multiply by relu'(x);
// relu 2 (max mode): relu' is encoded in the offsets (bit 7, see pool_fwd), x is not read.
// db (VEC 8 only, nullable): also db[c] += sum over pixels of dx[.][c] -- the bias
// gradient of the conv that produced x, folded in so that dx is never re-read.  The
// launch makes gridDim.x*NT a multiple of C/8, so each thread keeps one channel group.
template <int VEC>
__global__ void pool_bwd(const bf16_t *__restrict__ x, const uint8_t *__restrict__ arg, const bf16_t *__restrict__ dy,
                         bf16_t *__restrict__ dx, int N, int H, int W, int C, int Ho, int Wo, int KH, int KW, int S,
                         int P, int mode, int relu, float *__restrict__ db) {
  const int CV = C / VEC;
  const long total = static_cast<long>(N) * H * W * CV;
  const float inv = 1.0f / (KH * KW);
  float bsum[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) bsum[e] = 0.f;
  for (long idx = grid_stride_start(); idx < total; idx += grid_stride()) {
    const int cv = idx % CV;
    long t = idx / CV;
    const int w = t % W; t /= W;
    const int h = t % H;
    const int n = t / H;
    float xv[VEC], g[VEC];
    if (relu == 1) {
      if constexpr (VEC == 8) unpack8(*reinterpret_cast<const uint4 *>(x + idx * VEC), xv);
      else xv[0] = bf2f(x[idx]);
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) g[e] = 0.f;
    // windows ho with ho*S - P <= h < ho*S - P + KH
    const int hlo = max(0, (h + P - KH + S) / S), hhi = min(Ho - 1, (h + P) / S);
    const int wlo = max(0, (w + P - KW + S) / S), whi = min(Wo - 1, (w + P) / S);
    for (int ho = hlo; ho <= hhi; ++ho)
      for (int wo = wlo; wo <= whi; ++wo) {
        const long o = ((static_cast<long>(n) * Ho + ho) * Wo + wo) * C + cv * VEC;
        const uint32_t off = static_cast<uint32_t>((h - (ho * S - P)) * KW + (w - (wo * S - P)));
        float gv[VEC];
        uint32_t am[VEC];
        if constexpr (VEC == 8) {
          unpack8(*reinterpret_cast<const uint4 *>(dy + o), gv);
          if (mode == 0) {
            const uint2 a2 = *reinterpret_cast<const uint2 *>(arg + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              am[e] = (a2.x >> (8 * e)) & 0xff;
              am[e + 4] = (a2.y >> (8 * e)) & 0xff;
            }
          }
        } else {
          gv[0] = bf2f(dy[o]);
          if (mode == 0) am[0] = arg[o];
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          if (mode == 0) g[e] += (am[e] == off) ? gv[e] : 0.f;
          else g[e] += mode == 2 ? gv[e] * inv : gv[e];
        }
      }
    if (relu == 1)
#pragma unroll
      for (int e = 0; e < VEC; ++e) g[e] = xv[e] > 0.f ? g[e] : 0.f;
    if constexpr (VEC == 8) {
      const uint4 packed = pack8(g);
      *reinterpret_cast<uint4 *>(dx + idx * VEC) = packed;
      if (db) {  // sum what was stored (bf16-rounded), like a separate pass would
        float r[8];
        unpack8(packed, r);
#pragma unroll
        for (int e = 0; e < 8; ++e) bsum[e] += r[e];
      }
    } else {
      dx[idx] = f2bf(g[0]);
    }
  }
  if constexpr (VEC == 8) {
    if (db) {
      extern __shared__ float red[];  // [C]
      for (int c = threadIdx.x; c < C; c += blockDim.x) red[c] = 0.f;
      __syncthreads();
      const int cv = static_cast<int>((static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x) % CV);
#pragma unroll
      for (int e = 0; e < 8; ++e) atomicAdd(&red[cv * 8 + e], bsum[e]);
      __syncthreads();
      // per-block partials (a second kernel sums them): thousands of blocks doing
      // atomics on the same C addresses serialise in L2
      for (int c = threadIdx.x; c < C; c += blockDim.x) db[static_cast<long>(blockIdx.x) * C + c] = red[c];
    }
  }
}

template <int SS, int KS>
__global__ void pool_bwd_rows(const bf16_t *__restrict__ x, const uint8_t *__restrict__ arg,
                              const bf16_t *__restrict__ dy, bf16_t *__restrict__ dx, int H, int W, int C, int Ho,
                              int Wo, int KHr, int KWr, int Sr, int P, int mode, int relu, FastDiv fd_cv,
                              FastDiv fd_row, FastDiv fd_h, uint32_t total) {
  const int S = SS > 0 ? SS : Sr, KH = KS > 0 ? KS : KHr, KW = KS > 0 ? KS : KWr;
  const int CV = C / 8;
  const uint32_t gidx = xcd_remap(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;  // as pool_fwd_rows
  if (gidx >= total) return;
  const int row = static_cast<int>(fdiv(gidx, fd_row));          // n * H + h
  const int e = static_cast<int>(gidx) - row * (W * CV);
  const int n = static_cast<int>(fdiv(static_cast<uint32_t>(row), fd_h)), h = row - n * H;
  const int w = static_cast<int>(fdiv(static_cast<uint32_t>(e), fd_cv));
  const int cv = e - w * CV;
  const long idx = (static_cast<long>(row) * W + w) * C + cv * 8;
  float xv[8], g[8];
  if (relu == 1) unpack8(*reinterpret_cast<const uint4 *>(x + idx), xv);
#pragma unroll
  for (int q = 0; q < 8; ++q) g[q] = 0.f;
  const int hlo = max(0, (h + P - KH + S) / S), hhi = min(Ho - 1, (h + P) / S);
  const int wlo = max(0, (w + P - KW + S) / S), whi = min(Wo - 1, (w + P) / S);
  const float inv = 1.0f / (KH * KW);
  const long nb = static_cast<long>(n) * Ho;
  auto take = [&](const uint4 d, const uint2 a2, int ho, int wo) {
    const uint32_t off = static_cast<uint32_t>((h - (ho * S - P)) * KW + (w - (wo * S - P)));
    float gv[8];
    unpack8(d, gv);
    if (mode == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        g[q] += (((a2.x >> (8 * q)) & 0xff) == off) ? gv[q] : 0.f;
        g[q + 4] += (((a2.y >> (8 * q)) & 0xff) == off) ? gv[q + 4] : 0.f;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) g[q] += mode == 2 ? gv[q] * inv : gv[q];
    }
  };
  if constexpr (KS > 0 && SS > 0) {
    // at most T x T windows cover one input pixel: issue every dy / argmax load first
    // (clamped, masked), then accumulate in the generic loop's order
    constexpr int T = (KS + SS - 1) / SS;
    uint4 d[T * T];
    uint2 a[T * T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
      for (int j = 0; j < T; ++j) {
        const long o = ((nb + min(hlo + i, Ho - 1)) * Wo + min(wlo + j, Wo - 1)) * C + cv * 8;
        d[i * T + j] = *reinterpret_cast<const uint4 *>(dy + o);
        if (mode == 0) a[i * T + j] = *reinterpret_cast<const uint2 *>(arg + o);
      }
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
      for (int j = 0; j < T; ++j)
        if (hlo + i <= hhi && wlo + j <= whi) take(d[i * T + j], a[i * T + j], hlo + i, wlo + j);
  } else {
    for (int ho = hlo; ho <= hhi; ++ho)
      for (int wo = wlo; wo <= whi; ++wo) {
        const long o = ((nb + ho) * Wo + wo) * C + cv * 8;
        take(*reinterpret_cast<const uint4 *>(dy + o),
             mode == 0 ? *reinterpret_cast<const uint2 *>(arg + o) : make_uint2(0u, 0u), ho, wo);
      }
  }
  if (relu == 1)
#pragma unroll
    for (int q = 0; q < 8; ++q) g[q] = xv[q] > 0.f ? g[q] : 0.f;
  *reinterpret_cast<uint4 *>(dx + idx) = pack8(g);
}

// Backward of pool_fwd_s1k3 (max mode) on strips of R input rows: the (R + 2) x 3 windows that
// cover the strip are read once each (dy + recorded offset) and routed to the strip's rows;
// contributions arrive in (ho, wo) order as in pool_bwd_rows.  relu 1: times relu'(x); relu 2:
// relu' is in the offsets' bit 7 (a marked window matches no tap).
template <int R>
__global__ void pool_bwd_s1k3(const bf16_t *__restrict__ x, const uint8_t *__restrict__ arg,
                              const bf16_t *__restrict__ dy, bf16_t *__restrict__ dx, int H, int W, int C, int Ho,
                              int Wo, int P, int relu, FastDiv fd_cv, FastDiv fd_row, FastDiv fd_hs, uint32_t total) {
  const int CV = C / 8, HS = (H + R - 1) / R;
  const uint32_t idx = xcd_remap(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int row = static_cast<int>(fdiv(idx, fd_row));  // n * HS + strip
  const int e = static_cast<int>(idx) - row * (W * CV);
  const int n = static_cast<int>(fdiv(static_cast<uint32_t>(row), fd_hs)), st = row - n * HS;
  const int w = static_cast<int>(fdiv(static_cast<uint32_t>(e), fd_cv));
  const int cv = e - w * CV;
  const int h0 = st * R;
  float g[R][8];
#pragma unroll
  for (int o = 0; o < R; ++o)
#pragma unroll
    for (int q = 0; q < 8; ++q) g[o][q] = 0.f;
  // window rows ho = h + P - kh for the strip's rows h0..h0+R-1: ho0 = h0 + P - 2 .. h0 + R - 1 + P
  const int hob = h0 + P - 2;
#pragma unroll
  for (int t = 0; t < R + 2; ++t) {
    const int ho = hob + t;
    if (ho < 0 || ho >= Ho) continue;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int wo = w + P - 2 + j;  // kw = w - (wo - P) = 2 - j
      if (wo < 0 || wo >= Wo) continue;
      const long o = ((static_cast<long>(n) * Ho + ho) * Wo + wo) * C + cv * 8;
      float gv[8];
      unpack8(*reinterpret_cast<const uint4 *>(dy + o), gv);
      const uint2 a2 = *reinterpret_cast<const uint2 *>(arg + o);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int kh = (h0 + r) - (ho - P);  // the input row's tap in window row ho
        if (kh < 0 || kh > 2) continue;
        const uint32_t off = static_cast<uint32_t>(kh * 3 + (2 - j));
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          g[r][q] += (((a2.x >> (8 * q)) & 0xff) == off) ? gv[q] : 0.f;
          g[r][q + 4] += (((a2.y >> (8 * q)) & 0xff) == off) ? gv[q + 4] : 0.f;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int h = h0 + r;
    if (h >= H) break;
    const long idx8 = ((static_cast<long>(n) * H + h) * W + w) * C + cv * 8;
    if (relu == 1) {
      float xv[8];
      unpack8(*reinterpret_cast<const uint4 *>(x + idx8), xv);
#pragma unroll
      for (int q = 0; q < 8; ++q) g[r][q] = xv[q] > 0.f ? g[r][q] : 0.f;
    }
    *reinterpret_cast<uint4 *>(dx + idx8) = pack8(g[r]);
  }
}

// Backward of the 3x3 stride-2 max pool (AlexNet's pools) on 2x2 input cells.  In padded
// coordinates hp = h + P, window ho covers hp in [2ho, 2ho + 2], so input rows 2i and 2i + 1 are
// covered by window rows {i - 1, i} and {i}: the 4 windows (i-1..i) x (j-1..j) hold every
// contribution to the cell's 4 pixels.  pool_bwd_rows loads up to 4 windows per PIXEL (16 per
// cell, 9 distinct), all from L2; here each window is loaded once (4 per cell) and the cell's
// 4 outputs are written -- the kernel becomes write-bound.  Contributions are summed in
// (ho, wo) order as in pool_bwd_rows, so both give the same bits.  relu as pool_bwd_s1k3.
__global__ void pool_bwd_s2k3(const bf16_t *__restrict__ x, const uint8_t *__restrict__ arg,
                              const bf16_t *__restrict__ dy, bf16_t *__restrict__ dx, int H, int W, int C, int Ho,
                              int Wo, int P, int relu, int i0, int j0, int WC, FastDiv fd_cv, FastDiv fd_row,
                              FastDiv fd_hc, uint32_t total) {
  const int CV = C / 8;
  const uint32_t idx = xcd_remap(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int row = static_cast<int>(fdiv(idx, fd_row));  // n * HC + cell row
  const int e = static_cast<int>(idx) - row * (WC * CV);
  const int n = static_cast<int>(fdiv(static_cast<uint32_t>(row), fd_hc));
  const int i = row - n * static_cast<int>(fd_hc.d) + i0;
  const int cj = static_cast<int>(fdiv(static_cast<uint32_t>(e), fd_cv));
  const int cv = e - cj * CV, j = cj + j0;
  uint4 d[2][2];
  uint2 a[2][2];
  bool ok[2][2];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int ho = i - 1 + p, wo = j - 1 + q;
      ok[p][q] = ho >= 0 && ho < Ho && wo >= 0 && wo < Wo;
      const long o = ((static_cast<long>(n) * Ho + min(max(ho, 0), Ho - 1)) * Wo + min(max(wo, 0), Wo - 1)) * C +
                     cv * 8;
      d[p][q] = *reinterpret_cast<const uint4 *>(dy + o);
      a[p][q] = *reinterpret_cast<const uint2 *>(arg + o);
    }
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int h = 2 * i + r - P, w = 2 * j + s - P;
      if (h < 0 || h >= H || w < 0 || w >= W) continue;
      float g[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) g[k] = 0.f;
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int kh = 2 + r - 2 * p, kw = 2 + s - 2 * q;  // tap of (h, w) in window (i-1+p, j-1+q)
          if (kh > 2 || kw > 2 || !ok[p][q]) continue;
          const uint32_t off = static_cast<uint32_t>(kh * 3 + kw);
          float gv[8];
          unpack8(d[p][q], gv);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            g[k] += (((a[p][q].x >> (8 * k)) & 0xff) == off) ? gv[k] : 0.f;
            g[k + 4] += (((a[p][q].y >> (8 * k)) & 0xff) == off) ? gv[k + 4] : 0.f;
          }
        }
      const long o = ((static_cast<long>(n) * H + h) * W + w) * C + cv * 8;
      if (relu == 1) {
        float xv[8];
        unpack8(*reinterpret_cast<const uint4 *>(x + o), xv);
#pragma unroll
        for (int k = 0; k < 8; ++k) g[k] = xv[k] > 0.f ? g[k] : 0.f;
      }
      *reinterpret_cast<uint4 *>(dx + o) = pack8(g);
    }
}
}  // namespace

int nn::pool_cells = 1;  // cxn_set_kernel_variant(0, v): 0 keeps pool_bwd_rows for the 3x3 / 2 max pool (A/B)
CXN_API int cxn_pool_bwd(const void *x, const void *arg, const void *dy, void *dx, int N, int H, int W, int C, int Ho,
                         int Wo, int KH, int KW, int S, int P, int mode, int relu, float *db, float *ws,
                         long ws_elems, void *stream) {
  if (C % 8 == 0 && db == nullptr) {
    const long total = static_cast<long>(N) * H * W * (C / 8);
    if (total >= (1L << 31)) return -2;  // fdiv (mulhi + n) stays exact below 2^31
#define CXN_POOL_BWD(SSV, KSV)                                                                                  \
  CXN_LAUNCH((pool_bwd_rows<SSV, KSV>), cdiv(total, NT), NT, 0, S_,                                                       \
      (const bf16_t *)x, (const uint8_t *)arg, (const bf16_t *)dy, (bf16_t *)dx, H, W, C, Ho, Wo, KH, KW, S, P, mode, \
      relu, make_fastdiv(static_cast<uint32_t>(C / 8)), make_fastdiv(static_cast<uint32_t>(W * (C / 8))),          \
      make_fastdiv(static_cast<uint32_t>(H)), static_cast<uint32_t>(total))
    const int sq = KH == KW ? KH : 0;
    if (S == 1 && sq == 3 && mode == 0 && P <= 2 && pool_strips) {
      static const int r_env = [] {  // CXN_POOL_S1K3_R: probe override of the strip height (2 / 4 / 8)
        const char *e = getenv("CXN_POOL_S1K3_R");
        return e != nullptr ? atoi(e) : 4;
      }();
#define CXN_S1K3(RV)                                                                                           \
  {                                                                                                            \
    constexpr int R = RV;                                                                                      \
    const int HS = (H + R - 1) / R;                                                                            \
    const long tot = static_cast<long>(N) * HS * W * (C / 8);                                                  \
    CXN_LAUNCH((pool_bwd_s1k3<R>), cdiv(tot, NT), NT, 0, S_, (const bf16_t *)x, (const uint8_t *)arg,          \
               (const bf16_t *)dy, (bf16_t *)dx, H, W, C, Ho, Wo, P, relu,                                     \
               make_fastdiv(static_cast<uint32_t>(C / 8)), make_fastdiv(static_cast<uint32_t>(W * (C / 8))),   \
               make_fastdiv(static_cast<uint32_t>(HS)), static_cast<uint32_t>(tot));                          \
  }
      if (r_env == 2) CXN_S1K3(2)
      else if (r_env == 8) CXN_S1K3(8)
      else CXN_S1K3(4)
#undef CXN_S1K3
    } else if (S == 2 && sq == 3 && mode == 0 && nn::pool_cells) {
      const int i0 = P / 2, j0 = P / 2;
      const int HC = (P + H - 1) / 2 - i0 + 1, WC = (P + W - 1) / 2 - j0 + 1;
      const long tot = static_cast<long>(N) * HC * WC * (C / 8);
      CXN_LAUNCH((pool_bwd_s2k3), cdiv(tot, NT), NT, 0, S_, 
          (const bf16_t *)x, (const uint8_t *)arg, (const bf16_t *)dy, (bf16_t *)dx, H, W, C, Ho, Wo, P, relu, i0,
          j0, WC, make_fastdiv(static_cast<uint32_t>(C / 8)), make_fastdiv(static_cast<uint32_t>(WC * (C / 8))),
          make_fastdiv(static_cast<uint32_t>(HC)), static_cast<uint32_t>(tot));
    } else if (S == 2 && sq == 3) CXN_POOL_BWD(2, 3);
    else if (S == 1 && sq == 3) CXN_POOL_BWD(1, 3);
    else if (S == 2 && sq == 2) CXN_POOL_BWD(2, 2);
    else CXN_POOL_BWD(0, 0);
#undef CXN_POOL_BWD
    RET;
  }
  if (C % 8 == 0) {
    const long total = static_cast<long>(N) * H * W * C / 8;
    int nb = nblocks(total);
    size_t shm = 0;
    if (db) {  // gridDim*NT must be a multiple of C/8 (fixed channel group per thread)
      const int cv = C / 8;
      int gcd = cv, b = NT;
      while (b) { const int t = gcd % b; gcd = b; b = t; }
      const int m = cv / gcd;
      nb = nb / m * m;
      if (nb < m) nb = m;
      shm = static_cast<size_t>(C) * sizeof(float);
    }
    if (db && (ws == nullptr || ws_elems < static_cast<long>(nb) * C)) return -2;
    CXN_LAUNCH((pool_bwd<8>), nb, NT, shm, S_, (const bf16_t *)x, (const uint8_t *)arg, (const bf16_t *)dy, (bf16_t *)dx, N, H,
                                     W, C, Ho, Wo, KH, KW, S, P, mode, relu, db ? ws : nullptr);
    if (db) nn::reduce_partials(ws, nb, C, db, stream);
  } else {
    if (db) return -2;
    CXN_LAUNCH((pool_bwd<1>), nblocks(static_cast<long>(N) * H * W * C), NT, 0, S_, 
        (const bf16_t *)x, (const uint8_t *)arg, (const bf16_t *)dy, (bf16_t *)dx, N, H, W, C, Ho, Wo, KH, KW, S, P,
        mode, relu, nullptr);
  }
  RET;
}

namespace {
// Max-unpool with the reference's tie semantics (src/layer/pooling_layer-inl.hpp:55-86,
// `unpool<red::maximum>`): EVERY input of a window that equals the window's max receives
// that window's gradient (pool_tie = all).  Gather form: one thread per input element sums
// over the windows covering it; y is the saved pooled output.  relu: the pooled values were
// max(relu(x)) and the gradient is masked by relu'(x).
__global__ void pool_bwd_tie_all(const bf16_t *__restrict__ x, const bf16_t *__restrict__ y,
                                 const bf16_t *__restrict__ dy, bf16_t *__restrict__ dx, int N, int H, int W, int C,
                                 int Ho, int Wo, int KH, int KW, int S, int P, int relu) {
  const long total = static_cast<long>(N) * H * W * C;
  for (long i = grid_stride_start(); i < total; i += grid_stride()) {
    const int c = static_cast<int>(i % C);
    const long pix = i / C;
    const int w = static_cast<int>(pix % W);
    const long nh = pix / W;
    const int h = static_cast<int>(nh % H);
    const int n = static_cast<int>(nh / H);
    float xv = bf2f(x[i]);
    if (relu) xv = fmaxf(xv, 0.f);
    // windows ho with ho*S - P <= h <= ho*S - P + KH - 1
    const int hp = h + P, wp = w + P;
    const int ho0 = hp - KH + 1 > 0 ? (hp - KH + 1 + S - 1) / S : 0, ho1 = min(Ho - 1, hp / S);
    const int wo0 = wp - KW + 1 > 0 ? (wp - KW + 1 + S - 1) / S : 0, wo1 = min(Wo - 1, wp / S);
    float g = 0.f;
    for (int ho = ho0; ho <= ho1; ++ho)
      for (int wo = wo0; wo <= wo1; ++wo) {
        const long o = ((static_cast<long>(n) * Ho + ho) * Wo + wo) * C + c;
        if (bf2f(y[o]) == xv) g += bf2f(dy[o]);
      }
    if (relu && !(bf2f(x[i]) > 0.f)) g = 0.f;
    dx[i] = f2bf(g);
  }
}
}  // namespace

CXN_API int cxn_pool_bwd_tie_all(const void *x, const void *y, const void *dy, void *dx, int N, int H, int W, int C,
                                 int Ho, int Wo, int KH, int KW, int S, int P, int relu, void *stream) {
  CXN_LAUNCH((pool_bwd_tie_all), nblocks(static_cast<long>(N) * H * W * C), NT, 0, S_, 
      (const bf16_t *)x, (const bf16_t *)y, (const bf16_t *)dy, (bf16_t *)dx, N, H, W, C, Ho, Wo, KH, KW, S, P, relu);
  RET;
}
