// layer_norm: per-position normalisation over the channels of an NHWC map (LayerNorm(C),
// channels-last; layers/extra.py LayerNormLayer).  The node is [rows][C] bf16, rows = B HW; per row
// mean and biased variance over C, y = (x - mean) rstd slope[c] + bias[c], fp32 arithmetic and one
// rounding at the store.
//
//   cxn_ln_fwd   one launch: y, and mean / rstd [rows] fp32 for the backward
//   cxn_ln_bwd   one launch for dx = rstd (slope g - s1 / C - xhat s2 / C) and per-block column
//                partials of sum g and sum g xhat, then a fixed-order merge onto gbias / gslope
//
// Geometry.  A row lives in the registers of L consecutive lanes of one wave, L a power of two up
// to 64, so a wave holds 64 / L rows and a block of 256 lanes RPB = 256 / L: at C = 96 twelve of
// 16 lanes hold one 16-byte vector each and a wave normalises four rows at once; at C = 768 a row
// is 96 vectors over 64 lanes.  Lane lr of a row holds units lr, lr + L, .. (VPL of them; a unit is
// 8 channels, one 16-byte access, when C % 8 == 0 -- the pointers must then be 16-byte aligned, as
// every node buffer is, or the call returns -1 -- else one channel: the scalar variant; C <= 2048
// vectorised, <= 1024 scalar, -1 beyond).  Row sums are xor-butterflies over the row's L lanes, the same
// order for every row.  The statistics take two passes over the registers -- the mean, then the sum
// of squares of the centred values -- never raw moments, so a large mean with a small spread keeps
// its variance.
//
// Backward.  Block b walks row groups b, b + P, .. (P blocks); a lane keeps the column sums of its
// own channels in registers over all of them, the RPB row slots of a block are summed through LDS
// in slot order into slab b of the workspace ([C] sum g xhat, then [C] sum g), and the merge launch
// adds the slabs in slab order.  No atomics: the same bits on every run.  A row's x and g are in
// registers before its dx is written, so dx may alias either.  dx null: parameter gradients only.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int PMAX = 512;       // backward: blocks (slabs) at most
constexpr int FWD_BLOCKS = 8192;

struct LnArgs {
  long rows, nrb;  // rows, row groups of RPB
  int C, U, L;     // channels, units per row, lanes per row
  float fC;        // C as a float: the means are true divisions (sum / C is exact where the mean is)
};

template <int VPL>
__device__ __forceinline__ float row_sum(const float (&v)[VPL], int L) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) s += v[i];
  for (int off = L >> 1; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  return s;
}

// the lane's units of one row as floats; units past the row (or of a row past the end) are zeros
template <bool VEC, int VPL>
__device__ __forceinline__ void load_units(const bf16_t *row, int lr, const LnArgs &a, bool ok,
                                           float (&f)[VPL][VEC ? 8 : 1]) {
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const int u = lr + v * a.L;
    const bool in = ok && u < a.U;
    if constexpr (VEC) {
      uint4 q = make_uint4(0, 0, 0, 0);
      if (in) q = *reinterpret_cast<const uint4 *>(row + u * 8);
      unpack8(q, f[v]);
    } else {
      f[v][0] = in ? bf2f(row[u]) : 0.f;
    }
  }
}

template <bool VEC, int VPL>
__device__ __forceinline__ void load_param(const float *p, int lr, const LnArgs &a, float (&f)[VPL][VEC ? 8 : 1]) {
  constexpr int UW = VEC ? 8 : 1;
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const int u = lr + v * a.L;
#pragma unroll
    for (int j = 0; j < UW; ++j) f[v][j] = u < a.U ? p[u * UW + j] : 0.f;
  }
}

template <bool VEC, int VPL>
__device__ __forceinline__ void store_units(bf16_t *row, int lr, const LnArgs &a, bool ok,
                                            const float (&f)[VPL][VEC ? 8 : 1]) {
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const int u = lr + v * a.L;
    if (ok && u < a.U) {
      if constexpr (VEC) *reinterpret_cast<uint4 *>(row + u * 8) = pack8(f[v]);
      else row[u] = f2bf(f[v][0]);
    }
  }
}

template <bool VEC, int VPL>
__global__ __launch_bounds__(NT) void ln_fwd(const bf16_t *__restrict__ x, bf16_t *__restrict__ y,
                                             const float *__restrict__ slope, const float *__restrict__ bias,
                                             float *__restrict__ mean, float *__restrict__ rstd, const LnArgs a,
                                             float eps) {
  constexpr int UW = VEC ? 8 : 1;
  const int t = threadIdx.x, sub = t / a.L, lr = t - sub * a.L, rpb = NT / a.L;
  float sl[VPL][UW], bi[VPL][UW];
  load_param<VEC, VPL>(slope, lr, a, sl);
  load_param<VEC, VPL>(bias, lr, a, bi);
  for (long rb = blockIdx.x; rb < a.nrb; rb += gridDim.x) {
    const long r = rb * rpb + sub;
    const bool ok = r < a.rows;
    const size_t base = static_cast<size_t>(ok ? r : 0) * a.C;
    float f[VPL][UW], part[VPL];
    load_units<VEC, VPL>(x + base, lr, a, ok, f);
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      part[v] = 0.f;
#pragma unroll
      for (int j = 0; j < UW; ++j) part[v] += f[v][j];
    }
    const float mu = row_sum<VPL>(part, a.L) / a.fC;
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      const bool in = lr + v * a.L < a.U;
      part[v] = 0.f;
#pragma unroll
      for (int j = 0; j < UW; ++j) {
        f[v][j] = in ? f[v][j] - mu : 0.f;
        part[v] = fmaf(f[v][j], f[v][j], part[v]);
      }
    }
    const float rs = 1.f / sqrtf(row_sum<VPL>(part, a.L) / a.fC + eps);
#pragma unroll
    for (int v = 0; v < VPL; ++v)
#pragma unroll
      for (int j = 0; j < UW; ++j) f[v][j] = fmaf(f[v][j] * rs, sl[v][j], bi[v][j]);
    store_units<VEC, VPL>(y + base, lr, a, ok, f);
    if (ok && lr == 0) {
      mean[r] = mu;
      rstd[r] = rs;
    }
  }
}

// slab b of ws: [C] sum g xhat, then [C] sum g, over the rows of block b
template <bool VEC, int VPL>
__global__ __launch_bounds__(NT) void ln_bwd(const bf16_t *g, const bf16_t *x, bf16_t *dx,
                                             const float *__restrict__ slope, const float *__restrict__ mean,
                                             const float *__restrict__ rstd, float *__restrict__ ws, const LnArgs a) {
  constexpr int UW = VEC ? 8 : 1;
  __shared__ float s_red[NT * 2 * UW];
  const int t = threadIdx.x, sub = t / a.L, lr = t - sub * a.L, rpb = NT / a.L;
  float sl[VPL][UW], sg[VPL][UW], sgx[VPL][UW];
  load_param<VEC, VPL>(slope, lr, a, sl);
#pragma unroll
  for (int v = 0; v < VPL; ++v)
#pragma unroll
    for (int j = 0; j < UW; ++j) sg[v][j] = sgx[v][j] = 0.f;
  for (long rb = blockIdx.x; rb < a.nrb; rb += gridDim.x) {
    const long r = rb * rpb + sub;
    const bool ok = r < a.rows;
    const size_t base = static_cast<size_t>(ok ? r : 0) * a.C;
    float gf[VPL][UW], xh[VPL][UW], p1[VPL], p2[VPL];
    load_units<VEC, VPL>(g + base, lr, a, ok, gf);
    load_units<VEC, VPL>(x + base, lr, a, ok, xh);
    const float mu = ok ? mean[r] : 0.f, rs = ok ? rstd[r] : 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      const bool in = lr + v * a.L < a.U;
      p1[v] = p2[v] = 0.f;
#pragma unroll
      for (int j = 0; j < UW; ++j) {
        xh[v][j] = in ? (xh[v][j] - mu) * rs : 0.f;
        sg[v][j] += gf[v][j];
        sgx[v][j] = fmaf(gf[v][j], xh[v][j], sgx[v][j]);
        gf[v][j] *= sl[v][j];
        p1[v] += gf[v][j];
        p2[v] = fmaf(gf[v][j], xh[v][j], p2[v]);
      }
    }
    if (dx) {
      const float m1 = row_sum<VPL>(p1, a.L) / a.fC, m2 = row_sum<VPL>(p2, a.L) / a.fC;
#pragma unroll
      for (int v = 0; v < VPL; ++v)
#pragma unroll
        for (int j = 0; j < UW; ++j) gf[v][j] = rs * (gf[v][j] - m1 - xh[v][j] * m2);
      store_units<VEC, VPL>(dx + base, lr, a, ok, gf);
    }
  }
  // the block's row slots, summed in slot order, one unit index at a time
  float *slab = ws + static_cast<size_t>(blockIdx.x) * 2 * a.C;
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
#pragma unroll
    for (int j = 0; j < UW; ++j) {
      s_red[t * 2 * UW + j] = sg[v][j];
      s_red[t * 2 * UW + UW + j] = sgx[v][j];
    }
    __syncthreads();
    for (int q = t; q < a.L * 2 * UW; q += NT) {
      const int ql = q / (2 * UW), k = q - ql * 2 * UW;
      float sum = 0.f;
      for (int s = 0; s < rpb; ++s) sum += s_red[(s * a.L + ql) * 2 * UW + k];
      const int u = ql + v * a.L;
      if (u < a.U) slab[(k < UW ? a.C : 0) + u * UW + (k < UW ? k : k - UW)] = sum;
    }
    __syncthreads();
  }
}

// gslope[c] += sum over the slabs of [c], gbias[c] += of [C + c], in slab order
__global__ __launch_bounds__(NT) void ln_merge(const float *__restrict__ ws, int P, int C, float *gslope,
                                               float *gbias) {
  const int e = blockIdx.x * NT + threadIdx.x;
  if (e >= 2 * C) return;
  float sum = 0.f;
  for (int p = 0; p < P; ++p) sum += ws[static_cast<size_t>(p) * 2 * C + e];
  if (e < C) gslope[e] += sum;
  else gbias[e - C] += sum;
}

// lanes per row and units per lane; false: C beyond what the register rows hold
static bool shape_of(int C, bool vec, int &U, int &L, int &VPL) {
  if (C < 1) return false;
  U = vec ? C / 8 : C;
  const int cap = vec ? 4 : 16;
  VPL = 1;
  while (VPL < cap && U > 64 * VPL) VPL *= 2;
  if (U > 64 * VPL) return false;
  const int per = (U + VPL - 1) / VPL;
  L = 1;
  while (L < per) L *= 2;
  return true;
}

static bool make_args(LnArgs &a, long rows, int C, bool vec, int &VPL) {
  if (rows < 1 || !shape_of(C, vec, a.U, a.L, VPL)) return false;
  const int rpb = NT / a.L;
  a.rows = rows;
  a.nrb = (rows + rpb - 1) / rpb;
  a.C = C;
  a.fC = static_cast<float>(C);
  return true;
}

static int slabs(long nrb) { return static_cast<int>(nrb < PMAX ? nrb : PMAX); }

#define CXN_LN_PICK(KER_, ...)                                         \
  do {                                                                 \
    if (vec) {                                                         \
      if (VPL == 1) CXN_LN_GO(KER_, true, 1, __VA_ARGS__);             \
      else if (VPL == 2) CXN_LN_GO(KER_, true, 2, __VA_ARGS__);        \
      else CXN_LN_GO(KER_, true, 4, __VA_ARGS__);                      \
    } else {                                                           \
      if (VPL == 1) CXN_LN_GO(KER_, false, 1, __VA_ARGS__);            \
      else if (VPL == 2) CXN_LN_GO(KER_, false, 2, __VA_ARGS__);       \
      else if (VPL == 4) CXN_LN_GO(KER_, false, 4, __VA_ARGS__);       \
      else if (VPL == 8) CXN_LN_GO(KER_, false, 8, __VA_ARGS__);       \
      else CXN_LN_GO(KER_, false, 16, __VA_ARGS__);                    \
    }                                                                  \
  } while (0)
#define CXN_LN_GO(KER_, VEC_, VPL_, ...) CXN_LAUNCH((KER_<VEC_, VPL_>), grid, NT, 0, S_, __VA_ARGS__)

}  // namespace

// Rows a block holds at C channels (vector variant when C % 8 == 0): 256 / L; 0: C not served.
CXN_API long cxn_ln_rows_per_block(int C) {
  int U, L, VPL;
  return shape_of(C, C % 8 == 0, U, L, VPL) ? NT / L : 0;
}

// fp32 workspace of cxn_ln_bwd: P slabs of 2 C floats
CXN_API long cxn_ln_ws_floats(long rows, int C) {
  const long rpb = cxn_ln_rows_per_block(C);
  if (rows < 1 || rpb < 1) return 0;
  return static_cast<long>(slabs((rows + rpb - 1) / rpb)) * 2 * C;
}

// y [rows][C] = (x - mean) rstd slope + bias per row; mean, rstd [rows] fp32 written.  y must not alias x.
CXN_API int cxn_ln_fwd(const void *x, void *y, const float *slope, const float *bias, float *mean, float *rstd,
                       long rows, int C, float eps, void *stream) {
  if (!x || !y || !slope || !bias || !mean || !rstd) return -1;
  const bool vec = C % 8 == 0;
  if (vec && !(aligned16(x) && aligned16(y))) return -1;
  LnArgs a;
  int VPL;
  if (!make_args(a, rows, C, vec, VPL)) return -1;
  const int grid = static_cast<int>(a.nrb < FWD_BLOCKS ? a.nrb : FWD_BLOCKS);
  const bf16_t *xp = static_cast<const bf16_t *>(x);
  bf16_t *yp = static_cast<bf16_t *>(y);
  CXN_LN_PICK(ln_fwd, xp, yp, slope, bias, mean, rstd, a, eps);
  RET;
}

// gslope += sum g xhat, gbias += sum g over the rows; dx (nullable; may alias x or g) = rstd (slope g
// - s1 / C - xhat s2 / C).  ws: fp32 workspace of ws_floats >= cxn_ln_ws_floats(rows, C); -2 when it
// is smaller.
CXN_API int cxn_ln_bwd(const void *g, const void *x, void *dx, const float *slope, float *gslope, float *gbias,
                       const float *mean, const float *rstd, float *ws, long ws_floats, long rows, int C,
                       void *stream) {
  if (!g || !x || !slope || !gslope || !gbias || !mean || !rstd) return -1;
  const bool vec = C % 8 == 0;
  if (vec && !(aligned16(x) && aligned16(g) && (!dx || aligned16(dx)))) return -1;
  LnArgs a;
  int VPL;
  if (!make_args(a, rows, C, vec, VPL)) return -1;
  const int P = slabs(a.nrb);
  if (!ws || static_cast<long>(P) * 2 * C > ws_floats) return -2;
  const int grid = P;
  const bf16_t *gp = static_cast<const bf16_t *>(g), *xp = static_cast<const bf16_t *>(x);
  bf16_t *dp = static_cast<bf16_t *>(dx);
  CXN_LN_PICK(ln_bwd, gp, xp, dp, slope, mean, rstd, ws, a);
  CXN_LAUNCH((ln_merge), (2 * C + NT - 1) / NT, NT, 0, S_, (const float *)ws, P, C, gslope, gbias);
  RET;
}
