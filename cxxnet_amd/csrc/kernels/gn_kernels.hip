// group_norm: per-sample normalisation over groups of channels (layers/extra.py GroupNormLayer).
// Tensors are [B][HW][C] bf16 with C contiguous; slope / bias are fp32 [C]; the statistics
// mean / rstd are fp32 [B][groups], group g of a sample owning channels [g Cg, (g + 1) Cg).
//
//   forward   gn_stats -> gn_finalize -> gn_apply                 (3 launches, no memset)
//   backward  gn_bwd_reduce -> gn_bwd_finalize [-> gn_bwd_apply]
//
// The row-walking kernels (stats, apply, bwd_reduce, bwd_apply) use the geometry of
// bn_ma_kernels.hip inside ONE sample: a lane owns V = 8 channels (one 16-byte access) when
// C % 8 == 0 and every buffer is 16-byte aligned, else V = 1, and walks the sample's HW rows; a
// block is GX channel lanes x RL row lanes; blockIdx.x = sample * P + row chunk, blockIdx.y covers
// the channel lanes beyond GX.  The cut of a sample into P chunks of rpb rows depends on HW and C
// alone, never on B, so a sample's statistics, y and dx are the same bits alone and in a batch.
//
// A lane never needs to know where the group boundaries fall among its channels: the walks reduce
// to per-(sample, chunk, channel) partials in a workspace, and the finalize kernels -- one wave per
// (sample, group) -- merge them over the chunks and the Cg channels of the group in a fixed order.
// Statistics: Welford per lane, Chan merges everywhere else.  No E[x^2] - E[x]^2, no atomics:
// the result is the same bits on every run.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int WV = 64;           // lanes of a wave: one (sample, group) item per wave in the finalize kernels
constexpr int IPB = NT / WV;     // items per finalize block
constexpr int FL = 32;           // partial lanes per channel in the per-channel sums of gn_bwd_finalize
constexpr int FC = 8;            // channels per block there (B P partials per channel: many lanes, few channels)
static_assert(FL * FC == NT, "gn_bwd_finalize's channel blocks are NT threads");
constexpr int PMAX_REDUCE = 64;  // chunks per sample the reductions aim for
constexpr int PMAX_APPLY = 2048; // blocks the element-wise passes aim for, over the whole batch

struct Geo {
  int V, G, GX, RL, ny, P;
  long rpb;
};

// rows: the HW rows of one sample; pmax_total: chunks (blocks) per sample to aim for
static Geo make_geo(long rows, int C, bool vec, long pmax_total) {
  Geo g;
  g.V = vec ? 8 : 1;
  g.G = C / g.V;
  g.GX = g.G < NT ? g.G : NT;
  g.RL = NT / g.GX;
  g.ny = (g.G + g.GX - 1) / g.GX;
  const long pmax = pmax_total / g.ny > 1 ? pmax_total / g.ny : 1;
  const long m = static_cast<long>(g.RL) * 8;  // at least 8 rows per lane: amortises the block merge
  const long even = (rows + pmax - 1) / pmax;
  g.rpb = even > m ? even : m;
  g.P = static_cast<int>((rows + g.rpb - 1) / g.rpb);
  return g;
}
// the element-wise passes carry no partial, so their cut may follow the batch
static Geo apply_geo(long B, long HW, int C, bool vec) { return make_geo(HW, C, vec, B < PMAX_APPLY ? PMAX_APPLY / B : 1); }

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

// (na, ma, M2a) <- merge with (nb, mb, M2b); either count may be 0
__device__ __forceinline__ void chan_merge(float &na, float &ma, float &m2a, float nb, float mb, float m2b) {
  const float n = na + nb;
  const float f = n > 0.f ? nb / n : 0.f;
  const float d = mb - ma;
  ma += d * f;
  m2a += m2b + d * d * na * f;
  na = n;
}

// a * b rounded to fp32 on its own, never contracted into a following add: gn_bwd_finalize and
// gn_bwd_apply both form slope g this way, so that a group of one element cancels to exactly 0
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float mul_sub_rn(float a, float b, float c) {
#pragma clang fp contract(off)
  const float p = a * b;
  return p - c;
}

struct Lane {
  int rl, cg;       // row lane, channel lane (of V channels)
  bool act;
  long r0, r1;      // the chunk's rows inside the sample
  size_t base;      // element offset of the sample
  int b, p;
};
__device__ __forceinline__ Lane lane_of(long HW, int C, int G, int GX, int RL, long rpb, int P) {
  Lane l;
  const int t = threadIdx.x;
  l.rl = t / GX;
  const int gl = t - l.rl * GX;
  l.cg = blockIdx.y * GX + gl;
  l.act = l.rl < RL && l.cg < G;
  l.b = blockIdx.x / P;
  l.p = blockIdx.x - l.b * P;
  l.r0 = static_cast<long>(l.p) * rpb;
  l.r1 = l.r0 + rpb < HW ? l.r0 + rpb : HW;
  l.base = static_cast<size_t>(l.b) * static_cast<size_t>(HW) * C;
  return l;
}

// per-channel view of the per-(sample, group) statistics
template <int V>
__device__ __forceinline__ void group_stats(const float *__restrict__ mean, const float *__restrict__ rstd, int b,
                                            int groups, int c0, FastDiv cg, float *mv, float *rs) {
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const size_t q = static_cast<size_t>(b) * groups + fdiv(static_cast<uint32_t>(c0 + j), cg);
    mv[j] = mean[q];
    rs[j] = rstd[q];
  }
}

// ------------------------------------------------------------------ statistics
// ws[b P + p][0][c] = mean, [1][c] = M2 of channel c over rows [p rpb, min(HW, (p + 1) rpb)) of sample b
template <int V>
__global__ __launch_bounds__(NT) void gn_stats(const bf16_t *__restrict__ x, float *__restrict__ ws, long HW, int C,
                                               int G, int GX, int RL, long rpb, int P) {
  __shared__ float s_mean[V][NT], s_m2[V][NT], s_n[NT];
  const Lane l = lane_of(HW, C, G, GX, RL, rpb, P);
  float n = 0.f, mean[V], m2[V];
#pragma unroll
  for (int j = 0; j < V; ++j) mean[j] = m2[j] = 0.f;
  if (l.act) {
    const bf16_t *p = x + l.base + static_cast<size_t>(l.cg) * V;
#pragma unroll 4
    for (long r = l.r0 + l.rl; r < l.r1; r += RL) {
      float f[V];
      load_v<V>(p + static_cast<size_t>(r) * C, f);
      n += 1.f;
      const float rn = 1.f / n;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float d = f[j] - mean[j];
        mean[j] += d * rn;
        m2[j] += d * (f[j] - mean[j]);
      }
    }
  }
  const int t = threadIdx.x;
  int s = 1;
  while (s < RL) s <<= 1;
  // pairwise over the row lanes: at step s lanes rl < s read slots rl + s >= s and write their own
  for (s >>= 1; s >= 1; s >>= 1) {
    s_n[t] = n;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      s_mean[j][t] = mean[j];
      s_m2[j][t] = m2[j];
    }
    __syncthreads();
    if (l.rl < s && l.rl + s < RL) {
      const int q = t + s * GX;
      const float nb = s_n[q];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float nn = n;
        chan_merge(nn, mean[j], m2[j], nb, s_mean[j][q], s_m2[j][q]);
      }
      n += nb;
    }
    __syncthreads();
  }
  if (l.act && l.rl == 0) {
    float *o = ws + static_cast<size_t>(blockIdx.x) * 2 * C + static_cast<size_t>(l.cg) * V;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      o[j] = mean[j];
      o[C + j] = m2[j];
    }
  }
}

// One wave per (sample, group): lane k merges entries k, k + 64, ... of the group's P x Cg partials
// (entry e = chunk e / Cg, channel e % Cg), then the lanes merge in a shuffle tree.
__global__ __launch_bounds__(NT) void gn_finalize(const float *__restrict__ ws, int P, long rpb, long HW, int C,
                                                  int groups, int Cg, long items, float eps,
                                                  float *__restrict__ mean_o, float *__restrict__ rstd_o) {
  const int lane = threadIdx.x % WV;
  const long item = static_cast<long>(blockIdx.x) * IPB + threadIdx.x / WV;
  if (item >= items) return;  // the whole wave leaves
  const long b = item / groups;
  const int g = static_cast<int>(item - b * groups);
  const float *w = ws + static_cast<size_t>(b) * P * 2 * C + static_cast<size_t>(g) * Cg;
  float n = 0.f, mean = 0.f, m2 = 0.f;
  const int E = P * Cg;
  for (int e = lane; e < E; e += WV) {
    const int p = e / Cg, j = e - p * Cg;
    const long lo = static_cast<long>(p) * rpb;
    const long hi = lo + rpb < HW ? lo + rpb : HW;
    const float *q = w + static_cast<size_t>(p) * 2 * C + j;
    chan_merge(n, mean, m2, static_cast<float>(hi - lo), q[0], q[C]);
  }
#pragma unroll
  for (int s = WV / 2; s >= 1; s >>= 1) {
    const float nb = __shfl_down(n, s, WV), mb = __shfl_down(mean, s, WV), qb = __shfl_down(m2, s, WV);
    chan_merge(n, mean, m2, nb, mb, qb);  // (lanes >= 64 - s merge garbage nobody reads)
  }
  if (lane != 0) return;
  const float var = m2 / (static_cast<float>(HW) * static_cast<float>(Cg));
  mean_o[item] = mean;
  rstd_o[item] = 1.f / sqrtf(var + eps);
}

// ------------------------------------------------------------------ normalise
// y = (x - mean) rstd slope + bias: x - mean first, so a group of one element gives bias exactly
template <int V>
__global__ __launch_bounds__(NT) void gn_apply(const bf16_t *__restrict__ x, bf16_t *__restrict__ y,
                                               const float *__restrict__ slope, const float *__restrict__ bias,
                                               const float *__restrict__ mean, const float *__restrict__ rstd, long HW,
                                               int C, int groups, FastDiv cg, int G, int GX, int RL, long rpb, int P) {
  const Lane l = lane_of(HW, C, G, GX, RL, rpb, P);
  if (!l.act) return;
  const int c0 = l.cg * V;
  float mv[V], a[V], bv[V];
  group_stats<V>(mean, rstd, l.b, groups, c0, cg, mv, a);
#pragma unroll
  for (int j = 0; j < V; ++j) {
    a[j] *= slope[c0 + j];
    bv[j] = bias[c0 + j];
  }
#pragma unroll 4
  for (long r = l.r0 + l.rl; r < l.r1; r += RL) {
    const size_t off = l.base + static_cast<size_t>(r) * C + c0;
    float f[V], o[V];
    load_v<V>(x + off, f);
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = fmaf(f[j] - mv[j], a[j], bv[j]);
    store_v<V>(y + off, o);
  }
}

// ------------------------------------------------------------------ backward
// ws[b P + p][0][c] = sum g, [1][c] = sum g xhat over the chunk's rows, xhat = (x - mean) rstd
template <int V>
__global__ __launch_bounds__(NT) void gn_bwd_reduce(const bf16_t *__restrict__ g, const bf16_t *__restrict__ x,
                                                    const float *__restrict__ mean, const float *__restrict__ rstd,
                                                    float *__restrict__ ws, long HW, int C, int groups, FastDiv cg,
                                                    int G, int GX, int RL, long rpb, int P) {
  __shared__ float s_g[V][NT], s_gx[V][NT];
  const Lane l = lane_of(HW, C, G, GX, RL, rpb, P);
  float sg[V], sgx[V];
#pragma unroll
  for (int j = 0; j < V; ++j) sg[j] = sgx[j] = 0.f;
  if (l.act) {
    const int c0 = l.cg * V;
    float mv[V], rs[V];
    group_stats<V>(mean, rstd, l.b, groups, c0, cg, mv, rs);
#pragma unroll 4
    for (long r = l.r0 + l.rl; r < l.r1; r += RL) {
      const size_t off = l.base + static_cast<size_t>(r) * C + c0;
      float gf[V], xf[V];
      load_v<V>(g + off, gf);
      load_v<V>(x + off, xf);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        sg[j] += gf[j];
        sgx[j] = fmaf(gf[j], (xf[j] - mv[j]) * rs[j], sgx[j]);
      }
    }
  }
  const int t = threadIdx.x;
  int s = 1;
  while (s < RL) s <<= 1;
  for (s >>= 1; s >= 1; s >>= 1) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      s_g[j][t] = sg[j];
      s_gx[j][t] = sgx[j];
    }
    __syncthreads();
    if (l.rl < s && l.rl + s < RL) {
      const int q = t + s * GX;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        sg[j] += s_g[j][q];
        sgx[j] += s_gx[j][q];
      }
    }
    __syncthreads();
  }
  if (l.act && l.rl == 0) {
    float *o = ws + static_cast<size_t>(blockIdx.x) * 2 * C + static_cast<size_t>(l.cg) * V;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      o[j] = sg[j];
      o[C + j] = sgx[j];
    }
  }
}

// Blocks [0, item_blocks): one wave per (sample, group), coef[b][g] = (s1 / m, s2 / m) with
// s1 = sum slope[c] A, s2 = sum slope[c] Bx over the group's chunks and channels, m = HW Cg.
// The blocks after them: FC channels each, gbias[c] += sum A, gslope[c] += sum Bx over every
// sample and chunk, FL lanes per channel over contiguous runs, merged in lane order.
__global__ __launch_bounds__(NT) void gn_bwd_finalize(const float *__restrict__ ws, int P, long B, long HW, int C,
                                                      int groups, int Cg, int item_blocks,
                                                      const float *__restrict__ slope, float *gslope, float *gbias,
                                                      float *__restrict__ coef) {
  __shared__ float s_g[FL][FC], s_gx[FL][FC];
  if (static_cast<int>(blockIdx.x) < item_blocks) {
    const int lane = threadIdx.x % WV;
    const long item = static_cast<long>(blockIdx.x) * IPB + threadIdx.x / WV;
    if (item >= B * groups) return;  // the whole wave leaves
    const long b = item / groups;
    const int g = static_cast<int>(item - b * groups);
    const float *w = ws + static_cast<size_t>(b) * P * 2 * C + static_cast<size_t>(g) * Cg;
    const float *sl = slope + static_cast<size_t>(g) * Cg;
    float s1 = 0.f, s2 = 0.f;
    const int E = P * Cg;
    for (int e = lane; e < E; e += WV) {
      const int p = e / Cg, j = e - p * Cg;
      const float *q = w + static_cast<size_t>(p) * 2 * C + j;
      s1 += mul_rn(sl[j], q[0]);
      s2 += mul_rn(sl[j], q[C]);
    }
#pragma unroll
    for (int s = WV / 2; s >= 1; s >>= 1) {
      s1 += __shfl_down(s1, s, WV);
      s2 += __shfl_down(s2, s, WV);
    }
    if (lane != 0) return;
    const float m = static_cast<float>(HW) * static_cast<float>(Cg);
    coef[2 * item] = s1 / m;
    coef[2 * item + 1] = s2 / m;
    return;
  }
  const int cl = threadIdx.x % FC, ln = threadIdx.x / FC;
  const int c = (static_cast<int>(blockIdx.x) - item_blocks) * FC + cl;
  const long Q = B * P;
  const long chunk = (Q + FL - 1) / FL;
  const long q0 = ln * chunk, q1 = q0 + chunk < Q ? q0 + chunk : Q;
  float sg = 0.f, sgx = 0.f;
  if (c < C) {
    // (the loads of an unrolled trip are independent of the sums: eight in flight per lane, one order)
#pragma unroll 8
    for (long q = q0; q < q1; ++q) {
      const float *w = ws + static_cast<size_t>(q) * 2 * C + c;
      sg += w[0];
      sgx += w[C];
    }
  }
  s_g[ln][cl] = sg;
  s_gx[ln][cl] = sgx;
  __syncthreads();
  if (ln != 0 || c >= C) return;
  for (int q = 1; q < FL; ++q) {
    sg += s_g[q][cl];
    sgx += s_gx[q][cl];
  }
  gslope[c] += sgx;
  gbias[c] += sg;
}

// dx = rstd ((slope g - s1 / m) - xhat s2 / m); dx may alias x or g: element-wise, both read before the write
template <int V>
__global__ __launch_bounds__(NT) void gn_bwd_apply(const bf16_t *g, const bf16_t *x, bf16_t *dx,
                                                   const float *__restrict__ slope, const float *__restrict__ mean,
                                                   const float *__restrict__ rstd, const float *__restrict__ coef,
                                                   long HW, int C, int groups, FastDiv cg, int G, int GX, int RL,
                                                   long rpb, int P) {
  const Lane l = lane_of(HW, C, G, GX, RL, rpb, P);
  if (!l.act) return;
  const int c0 = l.cg * V;
  float mv[V], rs[V], sl[V], k1[V], k2[V];
  group_stats<V>(mean, rstd, l.b, groups, c0, cg, mv, rs);
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const size_t q = static_cast<size_t>(l.b) * groups + fdiv(static_cast<uint32_t>(c0 + j), cg);
    sl[j] = slope[c0 + j];
    k1[j] = coef[2 * q];
    k2[j] = coef[2 * q + 1];
  }
#pragma unroll 4
  for (long r = l.r0 + l.rl; r < l.r1; r += RL) {
    const size_t off = l.base + static_cast<size_t>(r) * C + c0;
    float gf[V], xf[V], o[V];
    load_v<V>(g + off, gf);
    load_v<V>(x + off, xf);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float xh = (xf[j] - mv[j]) * rs[j];
      const float t = mul_sub_rn(sl[j], gf[j], k1[j]);
      o[j] = rs[j] * fmaf(-xh, k2[j], t);
    }
    store_v<V>(dx + off, o);
  }
}

static bool bad_shape(long B, long HW, int C, int groups) {
  return B < 1 || HW < 1 || C < 1 || groups < 1 || C % groups != 0 || B * static_cast<long>(groups) > (1L << 30) ||
         HW * (C / groups) > (1L << 24);  // (the element count of a group is carried in fp32)
}

}  // namespace


// Workspace floats for every batch up to B on either path: [B][P][2][C].
CXN_API long cxn_gn_ws_floats(long B, long HW, int C) {
  if (B < 1 || HW < 1 || C < 1) return 0;
  long p = make_geo(HW, C, false, PMAX_REDUCE).P;
  if (C % 8 == 0) {
    const long pv = make_geo(HW, C, true, PMAX_REDUCE).P;
    p = pv > p ? pv : p;
  }
  return B * p * 2 * C;
}

#define GN_DISPATCH(KER, GEO, ...)                                                                        \
  do {                                                                                                    \
    if (vec)                                                                                              \
      CXN_LAUNCH((KER<8>), dim3(static_cast<unsigned>(B * (GEO).P), (GEO).ny), NT, 0, S_, __VA_ARGS__, (GEO).G, \
                 (GEO).GX, (GEO).RL, (GEO).rpb, (GEO).P);                                                 \
    else                                                                                                  \
      CXN_LAUNCH((KER<1>), dim3(static_cast<unsigned>(B * (GEO).P), (GEO).ny), NT, 0, S_, __VA_ARGS__, (GEO).G, \
                 (GEO).GX, (GEO).RL, (GEO).rpb, (GEO).P);                                                 \
  } while (0)

// Forward, the same in training and inference.  x, y [B][HW][C] bf16 (y must not alias x: backward
// reads x again); mean, rstd [B][groups] receive the statistics.  ws_floats >= cxn_gn_ws_floats.
CXN_API int cxn_gn_fwd(const void *x, void *y, const float *slope, const float *bias, float *mean, float *rstd,
                       float *ws, long ws_floats, long B, long HW, int C, int groups, float eps, void *stream) {
  if (bad_shape(B, HW, C, groups)) return -1;
  const bool vec = C % 8 == 0 && aligned16(x) && aligned16(y);
  const int Cg = C / groups;
  const FastDiv cg = make_fastdiv(static_cast<uint32_t>(Cg));
  const Geo r = make_geo(HW, C, vec, PMAX_REDUCE);
  if (B * r.P * 2 * C > ws_floats || B * r.P > 0x7fffffffL) return -2;
  GN_DISPATCH(gn_stats, r, (const bf16_t *)x, ws, HW, C);
  const long items = B * groups;
  CXN_LAUNCH((gn_finalize), cdiv(items, IPB), NT, 0, S_, (const float *)ws, r.P, r.rpb, HW, C, groups, Cg, items, eps,
             mean, rstd);
  const Geo a = apply_geo(B, HW, C, vec);
  GN_DISPATCH(gn_apply, a, (const bf16_t *)x, (bf16_t *)y, slope, bias, (const float *)mean, (const float *)rstd, HW, C,
              groups, cg);
  RET;
}

// Backward from the statistics of the last forward.  dx null: weight gradients only; dx may alias
// x or g.  coef [B][groups][2].
CXN_API int cxn_gn_bwd(const void *g, const void *x, void *dx, const float *slope, float *gslope, float *gbias,
                       const float *mean, const float *rstd, float *coef, float *ws, long ws_floats, long B, long HW,
                       int C, int groups, void *stream) {
  if (bad_shape(B, HW, C, groups)) return -1;
  const bool vec = C % 8 == 0 && aligned16(g) && aligned16(x) && aligned16(dx);
  const int Cg = C / groups;
  const FastDiv cg = make_fastdiv(static_cast<uint32_t>(Cg));
  const Geo r = make_geo(HW, C, vec, PMAX_REDUCE);
  if (B * r.P * 2 * C > ws_floats || B * r.P > 0x7fffffffL) return -2;
  GN_DISPATCH(gn_bwd_reduce, r, (const bf16_t *)g, (const bf16_t *)x, mean, rstd, ws, HW, C, groups, cg);
  const int item_blocks = cdiv(B * groups, IPB);
  CXN_LAUNCH((gn_bwd_finalize), item_blocks + (C + FC - 1) / FC, NT, 0, S_, (const float *)ws, r.P, B, HW, C, groups,
             Cg, item_blocks, slope, gslope, gbias, coef);
  if (!dx) RET;
  const Geo a = apply_geo(B, HW, C, vec);
  GN_DISPATCH(gn_bwd_apply, a, (const bf16_t *)g, (const bf16_t *)x, (bf16_t *)dx, slope, mean, rstd,
              (const float *)coef, HW, C, groups, cg);
  RET;
}
