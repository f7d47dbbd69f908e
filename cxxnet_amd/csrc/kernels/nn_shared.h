// What the memory-bound layer-family files share (layout_, pool_, lrn_, act_, loss_, reduce_ and
// copy_kernels.hip, and droppath_kernels.hip for dropout's threshold; nothing else includes this):
// the block size and grid-stride index of their
// kernels, the runtime value -> template argument dispatchers of their launchers, and the few
// host-side pieces one family's launchers need of another's.  No kernel lives here: a __global__
// function in a header would be emitted once per including file.
#pragma once
#include <type_traits>

#include "common.h"

constexpr int NT = 256;

__device__ __forceinline__ int grid_stride_start() { return blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ int grid_stride() { return gridDim.x * blockDim.x; }

// Runtime value -> template argument: f(std::integral_constant<int, h>) for the LRN half-window
// h = 0..4 (every caller has rejected larger windows; the default arm is 4), f(std::true_type /
// std::false_type) for a flag.  f is a generic lambda holding one CXN_LAUNCH.
template <typename F>
static inline void with_half(int half, F &&f) {
  switch (half) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}
template <typename F>
static inline void with_flag(bool on, F &&f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}
// dropout keeps element i iff hash_u32(i, seed) < pkeep * 2^32 (saturated)
static inline uint32_t dropout_thresh(float pkeep) {
  const double t = static_cast<double>(pkeep) * 4294967296.0;
  return t >= 4294967295.0 ? 0xFFFFFFFFu : static_cast<uint32_t>(t);
}

namespace nn {
// kernel variants kept for A/B (cxn_set_kernel_variant in reduce_kernels.hip,
// benchmarks/small_kernels.py), each defined in its family's file
extern int pool_cells;    // which = 0: pool_bwd_s2k3 cells (pool_kernels.hip)
extern int colsum_split;  // which = 1: colsum_multi column-chunk split (reduce_kernels.hip)
// db[c] += sum_b ws[b][c] over nb fp32 partial rows of C columns (reduce_kernels.hip
// partials_reduce); one fixed-order pass in deterministic mode
void reduce_partials(const float *ws, int nb, int C, float *db, void *stream);
}  // namespace nn
