// add: element-wise sum of 2-4 nodes with an optional fused relu (layers/extra.py AddLayer).
// Tensors are flat bf16 of n elements; the relu mask is ceil(n / 8) bytes, bit j of byte r =
// "element 8 r + j of the stored y is > 0".
//
//   forward   add_fwd   y = [relu](x0 + x1 (+ x2 + x3)), fp32 accumulation in input order, one
//                       rounding; with a mask pointer also the mask
//   backward  add_bwd   d_k = g where the mask bit is set, +0 elsewhere (no mask: d_k = g)
//
// Geometry: the unit of work is a run of 8 consecutive elements -- one 16-byte access per tensor
// and one mask byte -- and a run belongs to ONE thread on every path: the vector path (every
// pointer 16-byte aligned and n % 8 == 0) and the scalar path (2-byte accesses, the last run may
// be short).  So no two threads share a mask byte: no atomics, no cross-lane operations, no
// memset, the same bits on every run.  Blocks of 256 threads walk the runs with a grid stride;
// the grid is capped at 2048 blocks (8 per CU), which a memory-bound kernel needs to keep HBM busy.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_BLOCKS = 2048;

struct Src4 {
  const bf16_t *p[4];
};
struct Dst4 {
  bf16_t *p[4];
};

// cnt elements (8 on the vector path) of a run starting at p
template <bool VEC>
__device__ __forceinline__ void load_run(const bf16_t *p, int cnt, float *f) {
  if constexpr (VEC) {
    unpack8(*reinterpret_cast<const uint4 *>(p), f);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = j < cnt ? bf2f(p[j]) : 0.f;
  }
}

template <bool VEC>
__global__ __launch_bounds__(NT) void add_fwd(Src4 x, int n_in, bf16_t *__restrict__ y, uint8_t *__restrict__ mask,
                                              long n, long nrun, int relu) {
  const long stride = static_cast<long>(gridDim.x) * NT;
  for (long r = static_cast<long>(blockIdx.x) * NT + threadIdx.x; r < nrun; r += stride) {
    const long e0 = r * 8;
    const int cnt = VEC ? 8 : static_cast<int>(n - e0 < 8 ? n - e0 : 8);
    float acc[8], f[8];
    load_run<VEC>(x.p[0] + e0, cnt, acc);
#pragma unroll
    for (int k = 1; k < 4; ++k) {  // unrolled: constant indices into the by-value struct; n_in is uniform
      if (k < n_in) {
        load_run<VEC>(x.p[k] + e0, cnt, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += f[j];
      }
    }
    if (relu) {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = acc[j] > 0.f ? acc[j] : 0.f;
    }
    // the mask is taken from the value as stored: a positive sum below bf16's range rounds to 0
    unsigned bits = 0;
    if constexpr (VEC) {
      const uint4 o = pack8(acc);
      *reinterpret_cast<uint4 *>(y + e0) = o;
      unpack8(o, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) bits |= (f[j] > 0.f ? 1u : 0u) << j;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (j < cnt) {
          const bf16_t o = f2bf(acc[j]);
          y[e0 + j] = o;
          bits |= (bf2f(o) > 0.f ? 1u : 0u) << j;
        }
      }
    }
    if (mask) mask[r] = static_cast<uint8_t>(bits);
  }
}

// keep the bf16 halves of a packed pair whose mask bits (lo, hi) are set; the others become +0
__device__ __forceinline__ uint32_t keep2(uint32_t w, unsigned m, int j) {
  return w & (((m >> j) & 1u ? 0x0000ffffu : 0u) | ((m >> (j + 1)) & 1u ? 0xffff0000u : 0u));
}

template <bool VEC>
__global__ __launch_bounds__(NT) void add_bwd(const bf16_t *__restrict__ g, const uint8_t *__restrict__ mask, Dst4 d,
                                              int n_out, long n, long nrun) {
  const long stride = static_cast<long>(gridDim.x) * NT;
  for (long r = static_cast<long>(blockIdx.x) * NT + threadIdx.x; r < nrun; r += stride) {
    const long e0 = r * 8;
    const unsigned m = mask ? mask[r] : 0xffu;
    if constexpr (VEC) {
      uint4 v = *reinterpret_cast<const uint4 *>(g + e0);
      v.x = keep2(v.x, m, 0);
      v.y = keep2(v.y, m, 2);
      v.z = keep2(v.z, m, 4);
      v.w = keep2(v.w, m, 6);
#pragma unroll
      for (int k = 0; k < 4; ++k)  // unrolled: constant indices into the by-value struct
        if (k < n_out) *reinterpret_cast<uint4 *>(d.p[k] + e0) = v;
    } else {
      const int cnt = static_cast<int>(n - e0 < 8 ? n - e0 : 8);
      bf16_t v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = j < cnt && ((m >> j) & 1u) ? g[e0 + j] : static_cast<bf16_t>(0);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k >= n_out) continue;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (j < cnt) d.p[k][e0 + j] = v[j];
      }
    }
  }
}

static inline int run_blocks(long nrun) { return nblocks(nrun, NT, MAX_BLOCKS); }

}  // namespace

// y = x0 + .. + x[n_in - 1], relu'd when relu != 0.  mask (nullable, ceil(n / 8) bytes): bit
// "stored y > 0" per element; null at inference and without relu.  y must not alias an input.
CXN_API int cxn_add_fwd(const void *x0, const void *x1, const void *x2, const void *x3, int n_in, void *y, void *mask,
                        long n, int relu, void *stream) {
  if (n_in < 2 || n_in > 4 || n < 1 || !y) return -1;
  Src4 x{{(const bf16_t *)x0, (const bf16_t *)x1, (const bf16_t *)x2, (const bf16_t *)x3}};
  bool vec = n % 8 == 0 && aligned16(y);
  for (int k = 0; k < 4; ++k) {
    if (k >= n_in) x.p[k] = nullptr;
    else if (!x.p[k]) return -1;
    else vec = vec && aligned16(x.p[k]);
  }
  const long nrun = (n + 7) / 8;
  if (vec)
    CXN_LAUNCH((add_fwd<true>), run_blocks(nrun), NT, 0, S_, x, n_in, (bf16_t *)y, (uint8_t *)mask, n, nrun, relu);
  else
    CXN_LAUNCH((add_fwd<false>), run_blocks(nrun), NT, 0, S_, x, n_in, (bf16_t *)y, (uint8_t *)mask, n, nrun, relu);
  RET;
}

// d_k = g masked by the forward's mask (null: plain fan-out), k < n_out.  No d_k may alias g.
CXN_API int cxn_add_bwd(const void *g, const void *mask, void *d0, void *d1, void *d2, void *d3, int n_out, long n,
                        void *stream) {
  if (n_out < 1 || n_out > 4 || n < 1 || !g) return -1;
  Dst4 d{{(bf16_t *)d0, (bf16_t *)d1, (bf16_t *)d2, (bf16_t *)d3}};
  bool vec = n % 8 == 0 && aligned16(g);
  for (int k = 0; k < 4; ++k) {
    if (k >= n_out) d.p[k] = nullptr;
    else if (!d.p[k]) return -1;
    else vec = vec && aligned16(d.p[k]);
  }
  const long nrun = (n + 7) / 8;
  if (vec)
    CXN_LAUNCH((add_bwd<true>), run_blocks(nrun), NT, 0, S_, (const bf16_t *)g, (const uint8_t *)mask, d, n_out, n, nrun);
  else
    CXN_LAUNCH((add_bwd<false>), run_blocks(nrun), NT, 0, S_, (const bf16_t *)g, (const uint8_t *)mask, d, n_out, n, nrun);
  RET;
}
