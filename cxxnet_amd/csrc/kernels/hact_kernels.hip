// relu6 / hsigmoid / hswish: the bounded activations of the mobile nets (layers/extra.py
// HardActLayer).  Tensors are flat bf16 of n elements; arithmetic is fp32 with one rounding at
// the store.  "Strictly inside" decides every breakpoint:
//
//   kind          x <= lo          lo < x < hi           x >= hi        (lo, hi)
//   0 relu6       y = +0           y = x                 y = 6          (0, 6)
//                 dx = 0           dx = g                dx = 0
//   1 hsigmoid    y = +0           y = (x + 3) / 6       y = 1          (-3, 3)
//                 dx = 0           dx = g / 6            dx = 0
//   2 hswish      y = 0            y = x (x + 3) / 6     y = x          (-3, 3)
//                 dx = 0           dx = g (2 x + 3) / 6  dx = g
//
//   forward   hact_fwd   y = f(x)
//   backward  hact_bwd   dx = g f'(x), the derivative taken from the INPUT x (hswish is not
//                        monotonic); dx may be x: a run's x and g are read before its dx is written
//
// The rows "y = x" and "dx = g" are selections, not products: a bf16 value widened to fp32 and
// rounded back keeps its bits.
//
// Geometry (that of add_kernels.hip): the unit of work is a run of 8 consecutive elements -- one
// 16-byte access per tensor -- and a run belongs to ONE thread on every path: the vector path (every
// pointer 16-byte aligned and n % 8 == 0) and the scalar path (2-byte accesses, the last run may
// be short).  No atomics, no LDS, no workspace: the same bits on every run.  Blocks of 256 threads
// walk the runs with a grid stride; the grid is capped at 2048 blocks (8 per CU), which a
// memory-bound kernel needs to keep HBM busy.  kind is a template parameter: no branch on it
// inside the element loop.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_BLOCKS = 2048;
constexpr int RELU6 = 0, HSIGMOID = 1, HSWISH = 2;
constexpr float SIXTH = 1.f / 6.f;

template <int KIND>
__device__ __forceinline__ float act(float x) {
  if constexpr (KIND == RELU6) return x <= 0.f ? 0.f : (x >= 6.f ? 6.f : x);
  if constexpr (KIND == HSIGMOID) return x <= -3.f ? 0.f : (x >= 3.f ? 1.f : (x + 3.f) * SIXTH);
  return x <= -3.f ? 0.f : (x >= 3.f ? x : x * ((x + 3.f) * SIXTH));
}

template <int KIND>
__device__ __forceinline__ float act_grad(float x, float g) {
  if constexpr (KIND == RELU6) return x > 0.f && x < 6.f ? g : 0.f;
  if constexpr (KIND == HSIGMOID) return x > -3.f && x < 3.f ? g * SIXTH : 0.f;
  return x <= -3.f ? 0.f : (x >= 3.f ? g : g * ((2.f * x + 3.f) * SIXTH));
}

template <int KIND, bool VEC>
__global__ __launch_bounds__(NT) void hact_fwd(const bf16_t *__restrict__ x, bf16_t *__restrict__ y, long n,
                                               long nrun) {
  const long stride = static_cast<long>(gridDim.x) * NT;
  for (long r = static_cast<long>(blockIdx.x) * NT + threadIdx.x; r < nrun; r += stride) {
    const long e0 = r * 8;
    if constexpr (VEC) {
      float f[8];
      unpack8(*reinterpret_cast<const uint4 *>(x + e0), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = act<KIND>(f[j]);
      *reinterpret_cast<uint4 *>(y + e0) = pack8(f);
    } else {
      const int cnt = static_cast<int>(n - e0 < 8 ? n - e0 : 8);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < cnt) y[e0 + j] = f2bf(act<KIND>(bf2f(x[e0 + j])));
    }
  }
}

// dx may alias x (never g): no __restrict__ on the two, and a run's loads all come before its stores
template <int KIND, bool VEC>
__global__ __launch_bounds__(NT) void hact_bwd(const bf16_t *x, const bf16_t *__restrict__ g, bf16_t *dx, long n,
                                               long nrun) {
  const long stride = static_cast<long>(gridDim.x) * NT;
  for (long r = static_cast<long>(blockIdx.x) * NT + threadIdx.x; r < nrun; r += stride) {
    const long e0 = r * 8;
    if constexpr (VEC) {
      float fx[8], fg[8];
      unpack8(*reinterpret_cast<const uint4 *>(x + e0), fx);
      unpack8(*reinterpret_cast<const uint4 *>(g + e0), fg);
#pragma unroll
      for (int j = 0; j < 8; ++j) fg[j] = act_grad<KIND>(fx[j], fg[j]);
      *reinterpret_cast<uint4 *>(dx + e0) = pack8(fg);
    } else {
      const int cnt = static_cast<int>(n - e0 < 8 ? n - e0 : 8);
      bf16_t v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = j < cnt ? f2bf(act_grad<KIND>(bf2f(x[e0 + j]), bf2f(g[e0 + j]))) : bf16_t(0);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < cnt) dx[e0 + j] = v[j];
    }
  }
}

template <int KIND>
void launch_fwd(bool vec, const bf16_t *x, bf16_t *y, long n, long nrun, void *stream) {
  const int grid = nblocks(nrun, NT, MAX_BLOCKS);
  if (vec) CXN_LAUNCH((hact_fwd<KIND, true>), grid, NT, 0, S_, x, y, n, nrun);
  else CXN_LAUNCH((hact_fwd<KIND, false>), grid, NT, 0, S_, x, y, n, nrun);
}

template <int KIND>
void launch_bwd(bool vec, const bf16_t *x, const bf16_t *g, bf16_t *dx, long n, long nrun, void *stream) {
  const int grid = nblocks(nrun, NT, MAX_BLOCKS);
  if (vec) CXN_LAUNCH((hact_bwd<KIND, true>), grid, NT, 0, S_, x, g, dx, n, nrun);
  else CXN_LAUNCH((hact_bwd<KIND, false>), grid, NT, 0, S_, x, g, dx, n, nrun);
}

}  // namespace

// Elements one pass of the capped grid covers (2048 blocks x 256 threads x 8): beyond it a thread
// makes a second grid-stride trip.
CXN_API long cxn_hact_pass_elems() { return static_cast<long>(MAX_BLOCKS) * NT * 8; }

// y = f(x), kind 0 relu6 / 1 hsigmoid / 2 hswish.  y must not alias x.
CXN_API int cxn_hact_fwd(const void *x, void *y, long n, int kind, void *stream) {
  if (!x || !y || n <= 0 || kind < RELU6 || kind > HSWISH) return -1;
  const bool vec = n % 8 == 0 && aligned16(x) && aligned16(y);
  const long nrun = (n + 7) / 8;
  const bf16_t *xp = static_cast<const bf16_t *>(x);
  bf16_t *yp = static_cast<bf16_t *>(y);
  if (kind == RELU6) launch_fwd<RELU6>(vec, xp, yp, n, nrun, stream);
  else if (kind == HSIGMOID) launch_fwd<HSIGMOID>(vec, xp, yp, n, nrun, stream);
  else launch_fwd<HSWISH>(vec, xp, yp, n, nrun, stream);
  RET;
}

// dx = g f'(x).  dx may alias x; it must not alias g.
CXN_API int cxn_hact_bwd(const void *x, const void *g, void *dx, long n, int kind, void *stream) {
  if (!x || !g || !dx || n <= 0 || kind < RELU6 || kind > HSWISH) return -1;
  const bool vec = n % 8 == 0 && aligned16(x) && aligned16(g) && aligned16(dx);
  const long nrun = (n + 7) / 8;
  const bf16_t *xp = static_cast<const bf16_t *>(x), *gp = static_cast<const bf16_t *>(g);
  bf16_t *dp = static_cast<bf16_t *>(dx);
  if (kind == RELU6) launch_bwd<RELU6>(vec, xp, gp, dp, n, nrun, stream);
  else if (kind == HSIGMOID) launch_bwd<HSIGMOID>(vec, xp, gp, dp, n, nrun, stream);
  else launch_bwd<HSWISH>(vec, xp, gp, dp, n, nrun, stream);
  RET;
}
