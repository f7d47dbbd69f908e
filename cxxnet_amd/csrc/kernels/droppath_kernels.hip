// drop_path (stochastic depth, per sample): the regulariser on the residual branches of the
// EfficientNets (layers/extra.py DropPathLayer).  The tensor is [B][n] bf16, n the elements of one
// sample, changed in place:
//
//   sample b is kept iff hash_u32(b, seed') < dropout_thresh(pkeep), seed' = hash_u32(*counter, seed)
//   (seed itself with a null counter) -- cxn_dropout's mask at element b (act_kernels.hip)
//   kept      x <- bf16(x * (1.0f / pkeep)): one fp32 product, one rounding
//   dropped   x <- +0, whatever it held (inf and NaN included): a selection, not x * 0; the sample is
//             stored WITHOUT being loaded
//
// The same call with the same seed and counter value in backward applies the forward's mask to the
// gradient, so no mask is stored; counter is read on the device, so a replayed HIP graph or launch
// list draws a new mask on every replay.
//
// Geometry: blockIdx.y walks the samples (a stride of gridDim.y, which is B up to the 65535 a grid
// allows), so the keep decision is uniform over a block and costs one hash per block and sample.
// Inside a sample the unit of work is a run of 8 consecutive elements owned by ONE thread: the
// vector path (n % 8 == 0 and the base 16-byte aligned, so every sample starts aligned) makes one
// 16-byte access per run; the scalar path makes 2-byte accesses and counts runs from the sample's
// own first element, the last one short, so a run never straddles two samples.  Blocks of 256
// threads walk a sample's runs with a stride of gridDim.x, capped at 2048 blocks per sample.  No
// atomics, no LDS, no workspace.
#include "nn_shared.h"

namespace {

constexpr int MAX_BLOCKS_X = 2048;
constexpr int MAX_BLOCKS_Y = 65535;

template <bool VEC>
__global__ __launch_bounds__(NT) void drop_path_apply(bf16_t *x, long B, long n, long nrun, uint32_t seed0,
                                                      const int *counter, uint32_t thresh, float scale) {
  const uint32_t seed = counter ? hash_u32(static_cast<uint32_t>(*counter), seed0) : seed0;
  const long stride = static_cast<long>(gridDim.x) * NT;
  for (long b = blockIdx.y; b < B; b += gridDim.y) {
    const bool keep = hash_u32(static_cast<uint32_t>(b), seed) < thresh;
    bf16_t *xs = x + b * n;
    for (long r = static_cast<long>(blockIdx.x) * NT + threadIdx.x; r < nrun; r += stride) {
      const long e0 = r * 8;
      if constexpr (VEC) {
        uint4 *p = reinterpret_cast<uint4 *>(xs + e0);
        if (keep) {
          float f[8];
          unpack8(*p, f);
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] *= scale;
          *p = pack8(f);
        } else {
          *p = make_uint4(0u, 0u, 0u, 0u);
        }
      } else {
        const int cnt = static_cast<int>(n - e0 < 8 ? n - e0 : 8);
        if (keep) {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (j < cnt) xs[e0 + j] = f2bf(bf2f(xs[e0 + j]) * scale);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (j < cnt) xs[e0 + j] = bf16_t(0);
        }
      }
    }
  }
}

}  // namespace

// Elements of ONE sample that a pass of the capped grid covers (2048 blocks x 256 threads x 8):
// beyond it a thread makes a second trip inside the sample.
CXN_API long cxn_drop_path_pass_elems() { return static_cast<long>(MAX_BLOCKS_X) * NT * 8; }

// x[B][n] in place: kept samples scaled by 1 / pkeep, dropped samples +0.  counter may be null.
CXN_API int cxn_drop_path(void *x, long B, long n, unsigned seed, const int *counter, float pkeep, void *stream) {
  if (!x || B <= 0 || n <= 0 || !(pkeep > 0.f) || pkeep > 1.f) return -1;
  const bool vec = n % 8 == 0 && aligned16(x);
  const long nrun = (n + 7) / 8;
  const dim3 grid(nblocks(nrun, NT, MAX_BLOCKS_X), static_cast<unsigned>(B < MAX_BLOCKS_Y ? B : MAX_BLOCKS_Y));
  bf16_t *xp = static_cast<bf16_t *>(x);
  const uint32_t thresh = dropout_thresh(pkeep);
  const float scale = 1.0f / pkeep;
  if (vec) CXN_LAUNCH((drop_path_apply<true>), grid, NT, 0, S_, xp, B, n, nrun, seed, counter, thresh, scale);
  else CXN_LAUNCH((drop_path_apply<false>), grid, NT, 0, S_, xp, B, n, nrun, seed, counter, thresh, scale);
  RET;
}
