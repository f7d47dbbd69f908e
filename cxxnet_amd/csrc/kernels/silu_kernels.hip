// silu (swish-1), y = x sigma(x) with sigma(x) = 1 / (1 + e^-x): the activation of the EfficientNets
// (layers/extra.py SiluLayer).  Tensors are flat bf16 of n elements; arithmetic is fp32 with one
// rounding at the store.
//
//   forward   silu_fwd   y = x s,                    s = 1 / (1 + e),  e = e^-x
//   backward  silu_bwd   dx = g s (1 + x (1 - s)),   the derivative taken from the INPUT x (silu is
//                        not monotonic: its output cannot stand in for x); dx may be x: a run's x
//                        and g are read before its dx is written
//
// s is formed as 1 / (1 + e), never e' / (1 + e'): that keeps both ends finite.
//   x -> -inf   e overflows to +inf, s = +0: y = x 0 = -0 and dx = g 0 (1 + x) = a zero
//   x -> +inf   e underflows to 0, s = 1 exactly: y = x 1 and dx = g 1 (1 + x 0), the bits of x and g
// e is one v_exp_f32 of -x log2(e) and the reciprocal one v_rcp_f32, each within one ulp; neither
// produces subnormals, so for x <= -87 or so, where s is below fp32's normal range, s is +0.
//
// Geometry (that of hact_kernels.hip): the unit of work is a run of 8 consecutive elements -- one
// 16-byte access per tensor -- and a run belongs to ONE thread on every path: the vector path (every
// pointer 16-byte aligned and n % 8 == 0) and the scalar path (2-byte accesses, the last run may
// be short).  No atomics, no LDS, no workspace: the same bits on every run.  Blocks of 256 threads
// walk the runs with a grid stride; the grid is capped at 2048 blocks (8 per CU).
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_BLOCKS = 2048;
constexpr float NEG_LOG2E = -1.44269504088896340736f;

__device__ __forceinline__ float sigma(float x) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * NEG_LOG2E));
}

__device__ __forceinline__ float silu(float x) { return x * sigma(x); }

__device__ __forceinline__ float silu_grad(float x, float g) {
  const float s = sigma(x);
  return g * s * (1.f + x * (1.f - s));
}

template <bool VEC>
__global__ __launch_bounds__(NT) void silu_fwd(const bf16_t *__restrict__ x, bf16_t *__restrict__ y, long n,
                                               long nrun) {
  const long stride = static_cast<long>(gridDim.x) * NT;
  for (long r = static_cast<long>(blockIdx.x) * NT + threadIdx.x; r < nrun; r += stride) {
    const long e0 = r * 8;
    if constexpr (VEC) {
      float f[8];
      unpack8(*reinterpret_cast<const uint4 *>(x + e0), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = silu(f[j]);
      *reinterpret_cast<uint4 *>(y + e0) = pack8(f);
    } else {
      const int cnt = static_cast<int>(n - e0 < 8 ? n - e0 : 8);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < cnt) y[e0 + j] = f2bf(silu(bf2f(x[e0 + j])));
    }
  }
}

// dx may alias x (never g): no __restrict__ on the two, and a run's loads all come before its stores
template <bool VEC>
__global__ __launch_bounds__(NT) void silu_bwd(const bf16_t *x, const bf16_t *__restrict__ g, bf16_t *dx, long n,
                                               long nrun) {
  const long stride = static_cast<long>(gridDim.x) * NT;
  for (long r = static_cast<long>(blockIdx.x) * NT + threadIdx.x; r < nrun; r += stride) {
    const long e0 = r * 8;
    if constexpr (VEC) {
      float fx[8], fg[8];
      unpack8(*reinterpret_cast<const uint4 *>(x + e0), fx);
      unpack8(*reinterpret_cast<const uint4 *>(g + e0), fg);
#pragma unroll
      for (int j = 0; j < 8; ++j) fg[j] = silu_grad(fx[j], fg[j]);
      *reinterpret_cast<uint4 *>(dx + e0) = pack8(fg);
    } else {
      const int cnt = static_cast<int>(n - e0 < 8 ? n - e0 : 8);
      bf16_t v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = j < cnt ? f2bf(silu_grad(bf2f(x[e0 + j]), bf2f(g[e0 + j]))) : bf16_t(0);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < cnt) dx[e0 + j] = v[j];
    }
  }
}

}  // namespace

// Elements one pass of the capped grid covers (2048 blocks x 256 threads x 8): beyond it a thread
// makes a second grid-stride trip.
CXN_API long cxn_silu_pass_elems() { return static_cast<long>(MAX_BLOCKS) * NT * 8; }

// y = x sigma(x).  y must not alias x.
CXN_API int cxn_silu_fwd(const void *x, void *y, long n, void *stream) {
  if (!x || !y || n <= 0) return -1;
  const bool vec = n % 8 == 0 && aligned16(x) && aligned16(y);
  const long nrun = (n + 7) / 8;
  const int grid = nblocks(nrun, NT, MAX_BLOCKS);
  const bf16_t *xp = static_cast<const bf16_t *>(x);
  bf16_t *yp = static_cast<bf16_t *>(y);
  if (vec) CXN_LAUNCH((silu_fwd<true>), grid, NT, 0, S_, xp, yp, n, nrun);
  else CXN_LAUNCH((silu_fwd<false>), grid, NT, 0, S_, xp, yp, n, nrun);
  RET;
}

// dx = g silu'(x).  dx may alias x; it must not alias g.
CXN_API int cxn_silu_bwd(const void *x, const void *g, void *dx, long n, void *stream) {
  if (!x || !g || !dx || n <= 0) return -1;
  const bool vec = n % 8 == 0 && aligned16(x) && aligned16(g) && aligned16(dx);
  const long nrun = (n + 7) / 8;
  const int grid = nblocks(nrun, NT, MAX_BLOCKS);
  const bf16_t *xp = static_cast<const bf16_t *>(x), *gp = static_cast<const bf16_t *>(g);
  bf16_t *dp = static_cast<bf16_t *>(dx);
  if (vec) CXN_LAUNCH((silu_bwd<true>), grid, NT, 0, S_, xp, gp, dp, n, nrun);
  else CXN_LAUNCH((silu_bwd<false>), grid, NT, 0, S_, xp, gp, dp, n, nrun);
  RET;
}
