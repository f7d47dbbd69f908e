// gelu, the exact (erf) form: y = x Phi(x), Phi(x) = (1 + erf(x / sqrt 2)) / 2, the activation of
// ConvNeXt and the transformers (layers/extra.py GeluLayer).  Tensors are flat bf16 of n elements;
// arithmetic is fp32 with one rounding at the store.
//
//   forward   gelu_fwd   y = x Phi(x)
//   backward  gelu_bwd   dx = g (Phi(x) + x phi(x)),  phi(x) = e^(-x x / 2) / sqrt(2 pi), the
//                        derivative taken from the INPUT x (gelu is not monotonic: its output cannot
//                        stand in for x); dx may be x: a run's x and g are read before its dx is written
//
// Phi is formed as erfc(-x / sqrt 2) / 2, never (1 + erf) / 2: the left tail keeps its relative
// accuracy instead of cancelling, and both ends stay finite.
//   x -> -inf   erfc underflows to +0: y = x 0 = -0; x x overflows to +inf, phi = e^-inf = 0, and
//               dx = g (0 + x 0) = a zero
//   x -> +inf   erfc = 2, Phi = 1 exactly: y = x 1, and dx = g (1 + x 0), the bits of x and g
//
// Geometry (that of silu_kernels.hip): the unit of work is a run of 8 consecutive elements -- one
// 16-byte access per tensor -- and a run belongs to ONE thread on every path: the vector path (every
// pointer 16-byte aligned and n % 8 == 0) and the scalar path (2-byte accesses, the last run may
// be short).  No atomics, no LDS, no workspace: the same bits on every run.  Blocks of 256 threads
// walk the runs with a grid stride; the grid is capped at 2048 blocks (8 per CU).
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_BLOCKS = 2048;
constexpr float NEG_RSQRT2 = -0.70710678118654752440f;
constexpr float RSQRT_2PI = 0.39894228040143267794f;

__device__ __forceinline__ float cdf(float x) { return 0.5f * erfcf(x * NEG_RSQRT2); }

__device__ __forceinline__ float gelu(float x) { return x * cdf(x); }

__device__ __forceinline__ float gelu_grad(float x, float g) {
  const float pdf = RSQRT_2PI * expf(-0.5f * (x * x));
  return g * (cdf(x) + x * pdf);
}

template <bool VEC>
__global__ __launch_bounds__(NT) void gelu_fwd(const bf16_t *__restrict__ x, bf16_t *__restrict__ y, long n,
                                               long nrun) {
  const long stride = static_cast<long>(gridDim.x) * NT;
  for (long r = static_cast<long>(blockIdx.x) * NT + threadIdx.x; r < nrun; r += stride) {
    const long e0 = r * 8;
    if constexpr (VEC) {
      float f[8];
      unpack8(*reinterpret_cast<const uint4 *>(x + e0), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = gelu(f[j]);
      *reinterpret_cast<uint4 *>(y + e0) = pack8(f);
    } else {
      const int cnt = static_cast<int>(n - e0 < 8 ? n - e0 : 8);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < cnt) y[e0 + j] = f2bf(gelu(bf2f(x[e0 + j])));
    }
  }
}

// dx may alias x (never g): no __restrict__ on the two, and a run's loads all come before its stores
template <bool VEC>
__global__ __launch_bounds__(NT) void gelu_bwd(const bf16_t *x, const bf16_t *__restrict__ g, bf16_t *dx, long n,
                                               long nrun) {
  const long stride = static_cast<long>(gridDim.x) * NT;
  for (long r = static_cast<long>(blockIdx.x) * NT + threadIdx.x; r < nrun; r += stride) {
    const long e0 = r * 8;
    if constexpr (VEC) {
      float fx[8], fg[8];
      unpack8(*reinterpret_cast<const uint4 *>(x + e0), fx);
      unpack8(*reinterpret_cast<const uint4 *>(g + e0), fg);
#pragma unroll
      for (int j = 0; j < 8; ++j) fg[j] = gelu_grad(fx[j], fg[j]);
      *reinterpret_cast<uint4 *>(dx + e0) = pack8(fg);
    } else {
      const int cnt = static_cast<int>(n - e0 < 8 ? n - e0 : 8);
      bf16_t v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = j < cnt ? f2bf(gelu_grad(bf2f(x[e0 + j]), bf2f(g[e0 + j]))) : bf16_t(0);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < cnt) dx[e0 + j] = v[j];
    }
  }
}

}  // namespace

// y = x Phi(x).  y must not alias x.
CXN_API int cxn_gelu_fwd(const void *x, void *y, long n, void *stream) {
  if (!x || !y || n <= 0) return -1;
  const bool vec = n % 8 == 0 && aligned16(x) && aligned16(y);
  const long nrun = (n + 7) / 8;
  const int grid = nblocks(nrun, NT, MAX_BLOCKS);
  const bf16_t *xp = static_cast<const bf16_t *>(x);
  bf16_t *yp = static_cast<bf16_t *>(y);
  if (vec) CXN_LAUNCH((gelu_fwd<true>), grid, NT, 0, S_, xp, yp, n, nrun);
  else CXN_LAUNCH((gelu_fwd<false>), grid, NT, 0, S_, xp, yp, n, nrun);
  RET;
}

// dx = g gelu'(x).  dx may alias x; it must not alias g.
CXN_API int cxn_gelu_bwd(const void *x, const void *g, void *dx, long n, void *stream) {
  if (!x || !g || !dx || n <= 0) return -1;
  const bool vec = n % 8 == 0 && aligned16(x) && aligned16(g) && aligned16(dx);
  const long nrun = (n + 7) / 8;
  const int grid = nblocks(nrun, NT, MAX_BLOCKS);
  const bf16_t *xp = static_cast<const bf16_t *>(x), *gp = static_cast<const bf16_t *>(g);
  bf16_t *dp = static_cast<bf16_t *>(dx);
  if (vec) CXN_LAUNCH((gelu_bwd<true>), grid, NT, 0, S_, xp, gp, dp, n, nrun);
  else CXN_LAUNCH((gelu_bwd<false>), grid, NT, 0, S_, xp, gp, dp, n, nrun);
  RET;
}
