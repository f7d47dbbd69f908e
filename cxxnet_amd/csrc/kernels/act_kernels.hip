// activations and dropout, element-wise on flat bf16 tensors of n elements (16-byte accesses, a
// scalar tail of n % 8 elements in block 0).
//
//   cxn_act_fwd / cxn_act_bwd   relu, sigmoid, tanh, xelu (reference src/layer/op.h,
//                               activation_layer-inl.hpp); backward in terms of the output y
//   cxn_dropout                 counter-hash mask, no mask storage (reference
//                               src/layer/dropout_layer-inl.hpp:44-57)
//
// Return 0, or -3 when the launch failed.
#include "nn_shared.h"

namespace {
// kind: 0 relu, 1 sigmoid, 2 tanh, 3 xelu(b).  Backward is written in terms of the
// forward OUTPUT y (the reference stores activations in place, src/layer/op.h:32-73).
__device__ __forceinline__ float act_f(int kind, float x, float b) {
  switch (kind) {
    case 0: return fmaxf(x, 0.f);
    case 1: return 1.f / (1.f + __expf(-x));
    case 2: return tanhf(x);
    default: return x > 0.f ? x : x / b;
  }
}
__device__ __forceinline__ float act_g(int kind, float y, float b) {
  switch (kind) {
    case 0: return y > 0.f ? 1.f : 0.f;
    case 1: return y * (1.f - y);
    case 2: return 1.f - y * y;
    default: return y > 0.f ? 1.f : 1.f / b;
  }
}

// y (and y2 when non-null, the reference's in-place write of the input node) = f(x)
__global__ void act_fwd(const bf16_t *__restrict__ x, bf16_t *y, bf16_t *y2, long n, int kind, float b) {
  const long n8 = n / 8;
  for (long i = grid_stride_start(); i < n8; i += grid_stride()) {
    float v[8];
    unpack8(reinterpret_cast<const uint4 *>(x)[i], v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = act_f(kind, v[e], b);
    const uint4 o = pack8(v);
    reinterpret_cast<uint4 *>(y)[i] = o;
    if (y2) reinterpret_cast<uint4 *>(y2)[i] = o;
  }
  if (blockIdx.x == 0 && threadIdx.x < n - n8 * 8) {
    const long i = n8 * 8 + threadIdx.x;
    const bf16_t o = f2bf(act_f(kind, bf2f(x[i]), b));
    y[i] = o;
    if (y2) y2[i] = o;
  }
}
__global__ void act_bwd(const bf16_t *y, const bf16_t *dy, bf16_t *dx, long n, int kind, float b) {
  const long n8 = n / 8;
  for (long i = grid_stride_start(); i < n8; i += grid_stride()) {
    float yv[8], g[8];
    unpack8(reinterpret_cast<const uint4 *>(y)[i], yv);
    unpack8(reinterpret_cast<const uint4 *>(dy)[i], g);
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] *= act_g(kind, yv[e], b);
    reinterpret_cast<uint4 *>(dx)[i] = pack8(g);
  }
  if (blockIdx.x == 0 && threadIdx.x < n - n8 * 8) {
    const long i = n8 * 8 + threadIdx.x;
    dx[i] = f2bf(bf2f(dy[i]) * act_g(kind, bf2f(y[i]), b));
  }
}
}  // namespace

CXN_API int cxn_act_fwd(const void *x, void *y, void *y2, long n, int kind, float b, void *stream) {
  CXN_LAUNCH((act_fwd), nblocks(n / 8 + 1), NT, 0, S_, (const bf16_t *)x, (bf16_t *)y, (bf16_t *)y2, n, kind, b);
  RET;
}
CXN_API int cxn_act_bwd(const void *y, const void *dy, void *dx, long n, int kind, float b, void *stream) {
  CXN_LAUNCH((act_bwd), nblocks(n / 8 + 1), NT, 0, S_, (const bf16_t *)y, (const bf16_t *)dy, (bf16_t *)dx, n, kind, b);
  RET;
}

namespace {
// keep iff hash(seed, i) < pkeep * 2^32; x *= keep / pkeep.  The same call with the same
// seed in backward regenerates the mask, so no mask tensor is stored.
__global__ void dropout_apply(const bf16_t *x, bf16_t *y, long n, uint32_t seed0, const int *counter,
                              uint32_t thresh, float scale) {
  // counter (device, nullable) lets a captured HIP graph draw a fresh mask every replay
  const uint32_t seed = counter ? hash_u32(static_cast<uint32_t>(*counter), seed0) : seed0;
  const long n8 = n / 8;
  if (blockIdx.x == 0 && threadIdx.x < n - n8 * 8) {
    const long i = n8 * 8 + threadIdx.x;
    y[i] = f2bf(hash_u32(static_cast<uint32_t>(i), seed) < thresh ? bf2f(x[i]) * scale : 0.f);
  }
  for (long i = grid_stride_start(); i < n8; i += grid_stride()) {
    float v[8];
    unpack8(reinterpret_cast<const uint4 *>(x)[i], v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t h = hash_u32(static_cast<uint32_t>(i * 8 + e), seed);
      v[e] = h < thresh ? v[e] * scale : 0.f;
    }
    reinterpret_cast<uint4 *>(y)[i] = pack8(v);
  }
}
}  // namespace

CXN_API int cxn_dropout(const void *x, void *y, long n, unsigned seed, const int *counter, float pkeep,
                        void *stream) {
  CXN_LAUNCH((dropout_apply), nblocks(n / 8 + 1), NT, 0, S_, (const bf16_t *)x, (bf16_t *)y, n, seed, counter,
             dropout_thresh(pkeep), 1.0f / pkeep);
  RET;
}
