// Squeeze-and-excitation primitives (layers/extra.py ChScaleLayer, ops/nn.py pool_forward).
// x, g, y, dx are [B][HW][C] bf16 with C contiguous; the gate s and its gradient ds are [B][C] bf16.
//
//   ch_scale forward   se_scale_fwd      y = x * s[b][c]                        (one launch)
//   ch_scale backward  se_scale_bwd      dx = g * s,  ds[b][c] = sum_hw g * x   (one pass over g, x)
//                      [-> se_merge]     when an image's map is cut into parts
//   global pooling     se_pool_fwd       y[b][c] = scale * sum_hw x             (sum / avg)
//                      [-> se_merge]
//
// Geometry, shared by the three: a lane owns one channel group -- V = 8 channels (one 16-byte
// access) when C % 8 == 0 and every pointer is 16-byte aligned, else V = 1 -- of one image and
// keeps it for its whole pixel walk, so its gate values are loaded once per image and stay in
// registers.  A block is GX group lanes x RL pixel lanes (GX = min(groups, 16), RL = 256 / GX):
// the lanes of one step read RL runs of GX * 16 contiguous bytes, one contiguous run when
// GX == groups.  grid = (parts, ceil(groups / GX), B): grid.x cuts the map's HW pixels into parts
// (the forward more finely than the reductions).
//
// Reductions: a lane sums its pixels in fp32 in pixel order, the RL pixel lanes of a block are
// summed pairwise through LDS, and with one part the block stores the rounded result itself.
// With several parts each block stores its fp32 sums to ws[part][b * C + c] and se_merge adds
// them in part order, scales and rounds once.  No atomics, no memset: the same bits on every run.
// The part count depends on the shape alone (se_parts).
//
// Aliasing: dx may alias x (a lane reads x and g of an element before it writes dx there), and
// ds may alias s: with one part the block that stores ds[b][c..] is the only one that reads
// s[b][c..], and its lanes read it before the block's first barrier; with several parts ds is
// stored by se_merge, a later launch.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int GX_MAX = 16;        // group lanes of a block: 16 x 16 B = 256 contiguous bytes per pixel
constexpr int TARGET_BLOCKS = 2048;  // 8 per CU
// A part holds at least this many pixels per pixel lane.  The forward, which only streams, is cut
// finer than the reductions, whose blocks end in an LDS sum and whose parts a second launch merges:
// at the SE-ResNet-18 sites for batch 64, 8 instead of 2 shortened the backward by a quarter to a
// third and the pooling by a third or more (docs/performance.md); 16 gained at 56 x 56 and lost at
// 28 x 28, 32 lost at both.
constexpr int FWD_MIN_PIX = 2;
constexpr int RED_MIN_PIX = 8;

struct Geo {
  int V, G, GX, RL, ny;
};
static Geo make_geo(int C, bool vec) {
  Geo g;
  g.V = vec ? 8 : 1;
  g.G = C / g.V;
  g.GX = g.G < GX_MAX ? g.G : GX_MAX;
  g.RL = NT / g.GX;
  g.ny = (g.G + g.GX - 1) / g.GX;
  return g;
}

// Parts an image's HW pixels are cut into: enough for TARGET_BLOCKS blocks, every part at least
// min_pix pixels per pixel lane.  From the shape alone: the lane geometry is that of the vector
// path whenever C % 8 == 0, whatever the pointers' alignment turns out to be.
static int se_parts(long B, long HW, int C, int min_pix) {
  const Geo g = make_geo(C, C % 8 == 0);
  const long base = B * g.ny;
  const long want = (TARGET_BLOCKS + base - 1) / base;
  const long most = HW / (static_cast<long>(min_pix) * g.RL);
  const long p = want < most ? want : most;
  return static_cast<int>(p < 1 ? 1 : p);
}

template <int V> __device__ __forceinline__ void load_v(const bf16_t *p, float *f);
template <> __device__ __forceinline__ void load_v<8>(const bf16_t *p, float *f) {
  unpack8(*reinterpret_cast<const uint4 *>(p), f);
}
template <> __device__ __forceinline__ void load_v<1>(const bf16_t *p, float *f) { f[0] = bf2f(*p); }
template <int V> __device__ __forceinline__ void store_v(bf16_t *p, const float *f);
template <> __device__ __forceinline__ void store_v<8>(bf16_t *p, const float *f) {
  *reinterpret_cast<uint4 *>(p) = pack8(f);
}
template <> __device__ __forceinline__ void store_v<1>(bf16_t *p, const float *f) { *p = f2bf(f[0]); }

struct Lane {
  int rl, grp;
  bool act;
  long p0, p1;    // this block's pixels [p0, p1) of image b
  size_t img;     // element offset of image b
  size_t col;     // element offset of the lane's channels in a [B][C] tensor
};
__device__ __forceinline__ Lane lane_of(long HW, int C, int V, int G, int GX, int RL, long ppb) {
  Lane l;
  const int t = threadIdx.x;
  l.rl = t / GX;
  l.grp = blockIdx.y * GX + (t - l.rl * GX);
  l.act = l.rl < RL && l.grp < G;
  l.p0 = static_cast<long>(blockIdx.x) * ppb;
  l.p1 = l.p0 + ppb < HW ? l.p0 + ppb : HW;
  l.img = static_cast<size_t>(blockIdx.z) * HW * C + static_cast<size_t>(l.grp) * V;
  l.col = static_cast<size_t>(blockIdx.z) * C + static_cast<size_t>(l.grp) * V;
  return l;
}

// acc <- the sum over the block's RL pixel lanes, in lanes rl == 0.  Pairwise in a fixed order:
// at step s lanes rl < s add the slots of lanes rl + s.  Every thread of the block calls it.
template <int V>
__device__ __forceinline__ void sum_pixel_lanes(float *acc, const Lane &l, int GX, int RL, float (*sm)[NT]) {
  const int t = threadIdx.x;
  int s = 1;
  while (s < RL) s <<= 1;
  for (s >>= 1; s >= 1; s >>= 1) {
#pragma unroll
    for (int j = 0; j < V; ++j) sm[j][t] = acc[j];
    __syncthreads();
    if (l.rl < s && l.rl + s < RL) {
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += sm[j][t + s * GX];
    }
    __syncthreads();
  }
}

// the block's sums: rounded to out[b][c] (one part, times scale) or as fp32 to ws[part][b][c]
template <int V>
__device__ __forceinline__ void put_sums(float *acc, const Lane &l, bf16_t *out, float *ws, size_t BC, float scale) {
  if (!l.act || l.rl != 0) return;
  if (gridDim.x == 1) {
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] *= scale;
    store_v<V>(out + l.col, acc);
  } else {
    float *w = ws + static_cast<size_t>(blockIdx.x) * BC + l.col;
    if constexpr (V == 8) {
      *reinterpret_cast<float4 *>(w) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      *reinterpret_cast<float4 *>(w + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    } else {
      w[0] = acc[0];
    }
  }
}

template <int V>
__global__ __launch_bounds__(NT) void se_scale_fwd(const bf16_t *__restrict__ x, const bf16_t *__restrict__ s,
                                                   bf16_t *__restrict__ y, long HW, int C, int G, int GX, int RL,
                                                   long ppb) {
  const Lane l = lane_of(HW, C, V, G, GX, RL, ppb);
  if (!l.act) return;
  float sv[V];
  load_v<V>(s + l.col, sv);
#pragma unroll 4
  for (long p = l.p0 + l.rl; p < l.p1; p += RL) {
    const size_t o = l.img + static_cast<size_t>(p) * C;
    float f[V];
    load_v<V>(x + o, f);
#pragma unroll
    for (int j = 0; j < V; ++j) f[j] *= sv[j];
    store_v<V>(y + o, f);
  }
}

// dx and ds may alias x and s: no __restrict__ on those four
template <int V>
__global__ __launch_bounds__(NT) void se_scale_bwd(const bf16_t *__restrict__ g, const bf16_t *x, const bf16_t *s,
                                                   bf16_t *dx, bf16_t *ds, float *__restrict__ ws, long HW, int C,
                                                   int G, int GX, int RL, long ppb, size_t BC) {
  __shared__ float sm[V][NT];
  const Lane l = lane_of(HW, C, V, G, GX, RL, ppb);
  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  if (l.act) {
    float sv[V];
    load_v<V>(s + l.col, sv);
#pragma unroll 4
    for (long p = l.p0 + l.rl; p < l.p1; p += RL) {
      const size_t o = l.img + static_cast<size_t>(p) * C;
      float gv[V], xv[V];
      load_v<V>(g + o, gv);
      load_v<V>(x + o, xv);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        acc[j] += gv[j] * xv[j];  // (contracted to an fma or not, the product of two bf16 is exact in fp32)
        gv[j] *= sv[j];
      }
      store_v<V>(dx + o, gv);
    }
  }
  sum_pixel_lanes<V>(acc, l, GX, RL, sm);  // its barriers stand between every read of s and the store of ds
  put_sums<V>(acc, l, ds, ws, BC, 1.f);
}

template <int V>
__global__ __launch_bounds__(NT) void se_pool_fwd(const bf16_t *__restrict__ x, bf16_t *__restrict__ y,
                                                  float *__restrict__ ws, long HW, int C, int G, int GX, int RL,
                                                  long ppb, size_t BC, float scale) {
  __shared__ float sm[V][NT];
  const Lane l = lane_of(HW, C, V, G, GX, RL, ppb);
  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  if (l.act) {
#pragma unroll 4
    for (long p = l.p0 + l.rl; p < l.p1; p += RL) {
      float f[V];
      load_v<V>(x + l.img + static_cast<size_t>(p) * C, f);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += f[j];
    }
  }
  sum_pixel_lanes<V>(acc, l, GX, RL, sm);
  put_sums<V>(acc, l, y, ws, BC, scale);
}

// out[i] = bf16(scale * (ws[0][i] + ws[1][i] + ...)), the parts added in order
__global__ __launch_bounds__(NT) void se_merge(const float *__restrict__ ws, bf16_t *__restrict__ out, size_t BC,
                                               int parts, float scale) {
  const size_t i = static_cast<size_t>(blockIdx.x) * NT + threadIdx.x;
  if (i >= BC) return;
  float a = ws[i];
  for (int p = 1; p < parts; ++p) a += ws[static_cast<size_t>(p) * BC + i];
  out[i] = f2bf(a * scale);
}

struct Plan {
  Geo g;
  int parts;
  long ppb;
  dim3 grid;
};
static Plan make_plan(long B, long HW, int C, bool vec, int min_pix = RED_MIN_PIX) {
  Plan p;
  p.g = make_geo(C, vec);
  p.parts = se_parts(B, HW, C, min_pix);
  p.ppb = (HW + p.parts - 1) / p.parts;
  p.parts = static_cast<int>((HW + p.ppb - 1) / p.ppb);  // (no empty last part; still the shape's alone)
  p.grid = dim3(p.parts, p.g.ny, static_cast<unsigned>(B));
  return p;
}
static inline bool bad_shape(long B, long HW, int C) { return B < 1 || B > 65535 || HW < 1 || C < 1; }

}  // namespace

// parts the reductions (ch_scale backward, pooling) cut an image's map into (1: a block stores its result itself, no workspace)
CXN_API int cxn_se_parts(long B, long HW, int C) {
  if (bad_shape(B, HW, C)) return -1;
  return make_plan(B, HW, C, C % 8 == 0).parts;
}

// fp32 workspace elements the reductions need for any batch 1..Bmax of this map (0: none)
CXN_API long cxn_se_ws_floats(long Bmax, long HW, int C) {
  if (bad_shape(Bmax, HW, C)) return -1;
  long n = 0;
  for (long b = 1; b <= Bmax; ++b) {
    const int parts = make_plan(b, HW, C, C % 8 == 0).parts;
    const long need = parts > 1 ? static_cast<long>(parts) * b * C : 0;
    n = need > n ? need : n;
  }
  return n;
}

// y[b][p][c] = x[b][p][c] * s[b][c].  y must not alias x or s.
CXN_API int cxn_ch_scale_fwd(const void *x, const void *s, void *y, long B, long HW, int C, void *stream) {
  if (bad_shape(B, HW, C) || !x || !s || !y) return -1;
  const bool vec = C % 8 == 0 && aligned16(x) && aligned16(s) && aligned16(y);
  const Plan p = make_plan(B, HW, C, vec, FWD_MIN_PIX);
  const Geo &g = p.g;
  if (vec)
    CXN_LAUNCH((se_scale_fwd<8>), p.grid, NT, 0, S_, (const bf16_t *)x, (const bf16_t *)s, (bf16_t *)y, HW, C, g.G,
               g.GX, g.RL, p.ppb);
  else
    CXN_LAUNCH((se_scale_fwd<1>), p.grid, NT, 0, S_, (const bf16_t *)x, (const bf16_t *)s, (bf16_t *)y, HW, C, g.G,
               g.GX, g.RL, p.ppb);
  RET;
}

// dx = g * s, ds[b][c] = sum over the map of g * x.  dx may alias x, ds may alias s; neither may
// alias g.  ws: cxn_se_ws_floats fp32 elements (ws_floats: its size; unused with one part).
CXN_API int cxn_ch_scale_bwd(const void *g_, const void *x, const void *s, void *dx, void *ds, float *ws,
                             long ws_floats, long B, long HW, int C, void *stream) {
  if (bad_shape(B, HW, C) || !g_ || !x || !s || !dx || !ds) return -1;
  const bool vec = C % 8 == 0 && aligned16(g_) && aligned16(x) && aligned16(s) && aligned16(dx) && aligned16(ds) &&
                   aligned16(ws);
  const Plan p = make_plan(B, HW, C, vec);
  const Geo &g = p.g;
  const size_t BC = static_cast<size_t>(B) * C;
  if (p.parts > 1 && (!ws || ws_floats < static_cast<long>(p.parts * BC))) return -2;
  if (vec)
    CXN_LAUNCH((se_scale_bwd<8>), p.grid, NT, 0, S_, (const bf16_t *)g_, (const bf16_t *)x, (const bf16_t *)s,
               (bf16_t *)dx, (bf16_t *)ds, ws, HW, C, g.G, g.GX, g.RL, p.ppb, BC);
  else
    CXN_LAUNCH((se_scale_bwd<1>), p.grid, NT, 0, S_, (const bf16_t *)g_, (const bf16_t *)x, (const bf16_t *)s,
               (bf16_t *)dx, (bf16_t *)ds, ws, HW, C, g.G, g.GX, g.RL, p.ppb, BC);
  if (p.parts > 1)
    CXN_LAUNCH((se_merge), cdiv(static_cast<long>(BC), NT), NT, 0, S_, (const float *)ws, (bf16_t *)ds, BC, p.parts,
               1.f);
  RET;
}

// y[b][c] = scale * sum over the map of x[b][.][c] (scale 1: sum pooling, 1 / HW as an fp32
// number: avg), fp32 sums in a fixed order, one rounding.  ws as in cxn_ch_scale_bwd.
CXN_API int cxn_global_pool_fwd(const void *x, void *y, float *ws, long ws_floats, long B, long HW, int C,
                                float scale, void *stream) {
  if (bad_shape(B, HW, C) || !x || !y) return -1;
  const bool vec = C % 8 == 0 && aligned16(x) && aligned16(y) && aligned16(ws);
  const Plan p = make_plan(B, HW, C, vec);
  const Geo &g = p.g;
  const size_t BC = static_cast<size_t>(B) * C;
  if (p.parts > 1 && (!ws || ws_floats < static_cast<long>(p.parts * BC))) return -2;
  if (vec)
    CXN_LAUNCH((se_pool_fwd<8>), p.grid, NT, 0, S_, (const bf16_t *)x, (bf16_t *)y, ws, HW, C, g.G, g.GX, g.RL, p.ppb,
               BC, scale);
  else
    CXN_LAUNCH((se_pool_fwd<1>), p.grid, NT, 0, S_, (const bf16_t *)x, (bf16_t *)y, ws, HW, C, g.G, g.GX, g.RL, p.ppb,
               BC, scale);
  if (p.parts > 1)
    CXN_LAUNCH((se_merge), cdiv(static_cast<long>(BC), NT), NT, 0, S_, (const float *)ws, (bf16_t *)y, BC, p.parts,
               scale);
  RET;
}
