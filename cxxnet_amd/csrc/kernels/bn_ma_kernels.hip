// batch_norm_ma: batch normalisation with running statistics (layers/extra.py BatchNormMALayer).
// Tensors are [rows][C] bf16 with C contiguous; per-channel tensors are fp32.
//
//   training forward   bn_ma_stats -> bn_ma_finalize -> bn_ma_apply        (3 launches, no memset)
//   inference forward  bn_ma_infer_coef -> bn_ma_apply
//   backward           bn_ma_bwd_reduce -> bn_ma_bwd_coef [-> bn_ma_bwd_apply]
//
// Geometry shared by the row-walking kernels (stats, apply, bwd_reduce, bwd_apply): a lane owns
// one channel group -- V = 8 channels (one 16-byte access) when C % 8 == 0 and every buffer is
// 16-byte aligned, else V = 1 -- and keeps it for its whole row walk, so the per-channel
// coefficients stay in registers and the inner loop has no division.  A block is GX group lanes
// x RL row lanes (GX = min(groups, 256), RL = 256 / GX): with GX == groups the 256 lanes of one
// step read one contiguous run of RL rows.  grid.y covers the groups beyond GX, grid.x the row
// chunks of rpb rows.
//
// Statistics: every lane runs Welford's update over its rows, the RL row lanes of a block are
// merged pairwise in LDS (Chan et al.), and the block writes its partial (mean, M2) -- the count
// follows from the geometry -- to a workspace; bn_ma_finalize merges the partials in a fixed
// order.  No E[x^2] - E[x]^2, no atomics: the result is the same bits on every run.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int FL = 8;    // partial lanes per channel in the C-sized merge kernels
constexpr int FC = 32;   // channels per block there

struct Geo {
  int V, G, GX, RL, ny, P;
  long rpb;
};

// pmax_total: blocks to aim for (stats / reductions: the partial count the C-sized merge reads)
static Geo make_geo(long rows, int C, bool vec, int pmax_total) {
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
constexpr int PMAX_REDUCE = 512, PMAX_APPLY = 2048;

// upper bound of P over every row count <= rows (P is not monotonic in rows past m * pmax)
static long max_partials(long rows, int C, bool vec) {
  const Geo g = make_geo(rows, C, vec, PMAX_REDUCE);
  const long pmax = PMAX_REDUCE / g.ny > 1 ? PMAX_REDUCE / g.ny : 1;
  const long byrows = (rows + static_cast<long>(g.RL) * 8 - 1) / (static_cast<long>(g.RL) * 8);
  return byrows < pmax ? byrows : pmax;
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

// (na, ma, M2a) <- merge with (nb, mb, M2b); either count may be 0
__device__ __forceinline__ void chan_merge(float &na, float &ma, float &m2a, float nb, float mb, float m2b) {
  const float n = na + nb;
  const float f = n > 0.f ? nb / n : 0.f;
  const float d = mb - ma;
  ma += d * f;
  m2a += m2b + d * d * na * f;
  na = n;
}

struct Lane {
  int rl, gl, grp;
  bool act;
  long r0, r1;
};
__device__ __forceinline__ Lane lane_of(long rows, int G, int GX, int RL, long rpb) {
  Lane l;
  const int t = threadIdx.x;
  l.rl = t / GX;
  l.gl = t - l.rl * GX;
  l.grp = blockIdx.y * GX + l.gl;
  l.act = l.rl < RL && l.grp < G;
  l.r0 = static_cast<long>(blockIdx.x) * rpb;
  l.r1 = l.r0 + rpb < rows ? l.r0 + rpb : rows;
  return l;
}

// ------------------------------------------------------------------ statistics
// ws[p][0][c] = mean, ws[p][1][c] = M2 of rows [p rpb, min(rows, (p + 1) rpb))
template <int V>
__global__ __launch_bounds__(NT) void bn_ma_stats(const bf16_t *__restrict__ x, float *__restrict__ ws, long rows,
                                                  int C, int G, int GX, int RL, long rpb) {
  __shared__ float s_mean[V][NT], s_m2[V][NT], s_n[NT];
  const Lane l = lane_of(rows, G, GX, RL, rpb);
  float n = 0.f, mean[V], m2[V];
#pragma unroll
  for (int j = 0; j < V; ++j) mean[j] = m2[j] = 0.f;
  if (l.act) {
    const bf16_t *p = x + static_cast<size_t>(l.grp) * V;
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
    float *o = ws + static_cast<size_t>(blockIdx.x) * 2 * C + static_cast<size_t>(l.grp) * V;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      o[j] = mean[j];
      o[C + j] = m2[j];
    }
  }
}

// stat: [5][C] = mean | var (biased) | inv | a = slope inv | b = bias - mean a
// running <- mom running + (1 - mom) batch  (rmean null: no update)
__global__ __launch_bounds__(FL * FC) void bn_ma_finalize(const float *__restrict__ ws, int P, long rpb, long rows, int C,
                                                           const float *__restrict__ slope, const float *__restrict__ bias,
                                                           float eps, float mom, float *__restrict__ stat, float *rmean,
                                                           float *rvar) {
  __shared__ float s_n[FL][FC], s_mean[FL][FC], s_m2[FL][FC];
  const int cl = threadIdx.x % FC, ln = threadIdx.x / FC;
  const int c = blockIdx.x * FC + cl;
  const int chunk = (P + FL - 1) / FL;
  const int p0 = ln * chunk, p1 = p0 + chunk < P ? p0 + chunk : P;
  float n = 0.f, mean = 0.f, m2 = 0.f;
  if (c < C) {
    for (int p = p0; p < p1; ++p) {
      const long lo = static_cast<long>(p) * rpb;
      const long hi = lo + rpb < rows ? lo + rpb : rows;
      const float *w = ws + static_cast<size_t>(p) * 2 * C + c;
      chan_merge(n, mean, m2, static_cast<float>(hi - lo), w[0], w[C]);
    }
  }
  s_n[ln][cl] = n;
  s_mean[ln][cl] = mean;
  s_m2[ln][cl] = m2;
  __syncthreads();
  if (ln != 0 || c >= C) return;
  for (int q = 1; q < FL; ++q) chan_merge(n, mean, m2, s_n[q][cl], s_mean[q][cl], s_m2[q][cl]);
  const float var = m2 / static_cast<float>(rows);
  const float inv = 1.f / sqrtf(var + eps);
  const float a = slope[c] * inv;
  stat[c] = mean;
  stat[C + c] = var;
  stat[2 * C + c] = inv;
  stat[3 * C + c] = a;
  stat[4 * C + c] = bias[c] - mean * a;
  if (rmean) {
    const float k = 1.f - mom;
    rmean[c] = mom * rmean[c] + k * mean;
    rvar[c] = mom * rvar[c] + k * var;
  }
}

// inference coefficients from the running statistics into stat[3], stat[4]
__global__ void bn_ma_infer_coef(const float *__restrict__ rmean, const float *__restrict__ rvar,
                                 const float *__restrict__ slope, const float *__restrict__ bias, float eps,
                                 float *__restrict__ stat, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float a = slope[c] * (1.f / sqrtf(rvar[c] + eps));
  stat[3 * C + c] = a;
  stat[4 * C + c] = bias[c] - rmean[c] * a;
}

// ------------------------------------------------------------------ normalise
// y = x a + b; xsave (nullable) = x.  y may alias x (self-loop): element-wise, read before write.
template <int V>
__global__ __launch_bounds__(NT) void bn_ma_apply(const bf16_t *x, bf16_t *y, bf16_t *xsave,
                                                  const float *__restrict__ a, const float *__restrict__ b, long rows,
                                                  int C, int G, int GX, int RL, long rpb) {
  const Lane l = lane_of(rows, G, GX, RL, rpb);
  if (!l.act) return;
  const size_t c0 = static_cast<size_t>(l.grp) * V;
  float av[V], bv[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    av[j] = a[c0 + j];
    bv[j] = b[c0 + j];
  }
#pragma unroll 4
  for (long r = l.r0 + l.rl; r < l.r1; r += RL) {
    const size_t off = static_cast<size_t>(r) * C + c0;
    float f[V], o[V];
    load_v<V>(x + off, f);
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = fmaf(f[j], av[j], bv[j]);
    if (xsave) store_v<V>(xsave + off, f);  // (bf16 -> fp32 -> bf16 is exact)
    store_v<V>(y + off, o);
  }
}

// ------------------------------------------------------------------ backward
// ws[p][0][c] = sum g, ws[p][1][c] = sum g (x - mean) over the block's rows
template <int V>
__global__ __launch_bounds__(NT) void bn_ma_bwd_reduce(const bf16_t *__restrict__ g, const bf16_t *__restrict__ x,
                                                       const float *__restrict__ mean, float *__restrict__ ws,
                                                       long rows, int C, int G, int GX, int RL, long rpb) {
  __shared__ float s_g[V][NT], s_gx[V][NT];
  const Lane l = lane_of(rows, G, GX, RL, rpb);
  float sg[V], sgx[V];
#pragma unroll
  for (int j = 0; j < V; ++j) sg[j] = sgx[j] = 0.f;
  if (l.act) {
    const size_t c0 = static_cast<size_t>(l.grp) * V;
    float mv[V];
#pragma unroll
    for (int j = 0; j < V; ++j) mv[j] = mean[c0 + j];
#pragma unroll 4
    for (long r = l.r0 + l.rl; r < l.r1; r += RL) {
      const size_t off = static_cast<size_t>(r) * C + c0;
      float gf[V], xf[V];
      load_v<V>(g + off, gf);
      load_v<V>(x + off, xf);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        sg[j] += gf[j];
        sgx[j] = fmaf(gf[j], xf[j] - mv[j], sgx[j]);
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
    float *o = ws + static_cast<size_t>(blockIdx.x) * 2 * C + static_cast<size_t>(l.grp) * V;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      o[j] = sg[j];
      o[C + j] = sgx[j];
    }
  }
}

// gslope += inv sum g (x - mean); gbias += sum g; dx = g A + (x - mean) B + Cc with
// A = slope inv, B = -A inv^2 sum g (x - mean) / R, Cc = -A sum g / R     (coef [3][C])
__global__ __launch_bounds__(FL * FC) void bn_ma_bwd_coef(const float *__restrict__ ws, int P, long rows, int C,
                                                           const float *__restrict__ stat,
                                                           const float *__restrict__ slope, float *gslope, float *gbias,
                                                           float *__restrict__ coef) {
  __shared__ float s_g[FL][FC], s_gx[FL][FC];
  const int cl = threadIdx.x % FC, ln = threadIdx.x / FC;
  const int c = blockIdx.x * FC + cl;
  const int chunk = (P + FL - 1) / FL;
  const int p0 = ln * chunk, p1 = p0 + chunk < P ? p0 + chunk : P;
  float sg = 0.f, sgx = 0.f;
  if (c < C) {
    for (int p = p0; p < p1; ++p) {
      const float *w = ws + static_cast<size_t>(p) * 2 * C + c;
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
  const float inv = stat[2 * C + c];
  const float A = slope[c] * inv;
  const float rr = 1.f / static_cast<float>(rows);
  gslope[c] += sgx * inv;
  gbias[c] += sg;
  coef[c] = A;
  coef[C + c] = -A * inv * inv * sgx * rr;
  coef[2 * C + c] = -A * sg * rr;
}

// dx may alias x or g: element-wise, both read before the write
template <int V>
__global__ __launch_bounds__(NT) void bn_ma_bwd_apply(const bf16_t *g, const bf16_t *x, bf16_t *dx,
                                                      const float *__restrict__ mean, const float *__restrict__ coef,
                                                      long rows, int C, int G, int GX, int RL, long rpb) {
  const Lane l = lane_of(rows, G, GX, RL, rpb);
  if (!l.act) return;
  const size_t c0 = static_cast<size_t>(l.grp) * V;
  float mv[V], A[V], B[V], Cc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    mv[j] = mean[c0 + j];
    A[j] = coef[c0 + j];
    B[j] = coef[C + c0 + j];
    Cc[j] = coef[2 * static_cast<size_t>(C) + c0 + j];
  }
#pragma unroll 4
  for (long r = l.r0 + l.rl; r < l.r1; r += RL) {
    const size_t off = static_cast<size_t>(r) * C + c0;
    float gf[V], xf[V], o[V];
    load_v<V>(g + off, gf);
    load_v<V>(x + off, xf);
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = fmaf(gf[j], A[j], fmaf(xf[j] - mv[j], B[j], Cc[j]));
    store_v<V>(dx + off, o);
  }
}

}  // namespace


// Workspace floats that cover every row count up to `rows` on either path.
CXN_API long cxn_bn_ma_ws_floats(long rows, int C) {
  if (rows < 1 || C < 1) return 0;
  long p = max_partials(rows, C, false);
  if (C % 8 == 0) {
    const long pv = max_partials(rows, C, true);
    p = pv > p ? pv : p;
  }
  return p * 2 * C;
}

// Training forward.  stat [5][C] (see bn_ma_finalize); xsave nullable (self-loop: y aliases x);
// rmean / rvar nullable (no running update).  ws: ws_floats >= cxn_bn_ma_ws_floats(rows, C).
CXN_API int cxn_bn_ma_fwd_train(const void *x, void *y, void *xsave, const float *slope, const float *bias,
                                float *stat, float *rmean, float *rvar, float *ws, long ws_floats, long rows, int C,
                                float eps, float mom, void *stream) {
  if (rows < 1 || C < 1) return -1;
  const bool vec = C % 8 == 0 && aligned16(x) && aligned16(y) && aligned16(xsave);
  const Geo g = make_geo(rows, C, vec, PMAX_REDUCE);
  if (static_cast<long>(g.P) * 2 * C > ws_floats) return -2;
  if (vec)
    CXN_LAUNCH((bn_ma_stats<8>), dim3(g.P, g.ny), NT, 0, S_, (const bf16_t *)x, ws, rows, C, g.G, g.GX, g.RL, g.rpb);
  else
    CXN_LAUNCH((bn_ma_stats<1>), dim3(g.P, g.ny), NT, 0, S_, (const bf16_t *)x, ws, rows, C, g.G, g.GX, g.RL, g.rpb);
  CXN_LAUNCH((bn_ma_finalize), (C + FC - 1) / FC, FL * FC, 0, S_, (const float *)ws, g.P, g.rpb, rows, C, slope, bias,
             eps, mom, stat, rmean, rvar);
  const Geo a = make_geo(rows, C, vec, PMAX_APPLY);
  if (vec)
    CXN_LAUNCH((bn_ma_apply<8>), dim3(a.P, a.ny), NT, 0, S_, (const bf16_t *)x, (bf16_t *)y, (bf16_t *)xsave,
               (const float *)(stat + 3 * static_cast<size_t>(C)), (const float *)(stat + 4 * static_cast<size_t>(C)),
               rows, C, a.G, a.GX, a.RL, a.rpb);
  else
    CXN_LAUNCH((bn_ma_apply<1>), dim3(a.P, a.ny), NT, 0, S_, (const bf16_t *)x, (bf16_t *)y, (bf16_t *)xsave,
               (const float *)(stat + 3 * static_cast<size_t>(C)), (const float *)(stat + 4 * static_cast<size_t>(C)),
               rows, C, a.G, a.GX, a.RL, a.rpb);
  RET;
}

// Inference forward: y = (x - rmean) / sqrt(rvar + eps) slope + bias; only stat[3], stat[4] are written.
CXN_API int cxn_bn_ma_fwd_infer(const void *x, void *y, const float *slope, const float *bias, const float *rmean,
                                const float *rvar, float *stat, long rows, int C, float eps, void *stream) {
  if (rows < 1 || C < 1) return -1;
  const bool vec = C % 8 == 0 && aligned16(x) && aligned16(y);
  CXN_LAUNCH((bn_ma_infer_coef), (C + NT - 1) / NT, NT, 0, S_, rmean, rvar, slope, bias, eps, stat, C);
  const Geo a = make_geo(rows, C, vec, PMAX_APPLY);
  if (vec)
    CXN_LAUNCH((bn_ma_apply<8>), dim3(a.P, a.ny), NT, 0, S_, (const bf16_t *)x, (bf16_t *)y, (bf16_t *)nullptr,
               (const float *)(stat + 3 * static_cast<size_t>(C)), (const float *)(stat + 4 * static_cast<size_t>(C)),
               rows, C, a.G, a.GX, a.RL, a.rpb);
  else
    CXN_LAUNCH((bn_ma_apply<1>), dim3(a.P, a.ny), NT, 0, S_, (const bf16_t *)x, (bf16_t *)y, (bf16_t *)nullptr,
               (const float *)(stat + 3 * static_cast<size_t>(C)), (const float *)(stat + 4 * static_cast<size_t>(C)),
               rows, C, a.G, a.GX, a.RL, a.rpb);
  RET;
}

// Backward from the stat of the last training forward.  dx null: weight gradients only.
// dx may alias x or g.  coef [3][C].
CXN_API int cxn_bn_ma_bwd(const void *g, const void *x, void *dx, const float *slope, float *gslope, float *gbias,
                          const float *stat, float *coef, float *ws, long ws_floats, long rows, int C,
                          void *stream) {
  if (rows < 1 || C < 1) return -1;
  const bool vec = C % 8 == 0 && aligned16(g) && aligned16(x) && aligned16(dx);
  const Geo r = make_geo(rows, C, vec, PMAX_REDUCE);
  if (static_cast<long>(r.P) * 2 * C > ws_floats) return -2;
  if (vec)
    CXN_LAUNCH((bn_ma_bwd_reduce<8>), dim3(r.P, r.ny), NT, 0, S_, (const bf16_t *)g, (const bf16_t *)x, stat, ws, rows,
               C, r.G, r.GX, r.RL, r.rpb);
  else
    CXN_LAUNCH((bn_ma_bwd_reduce<1>), dim3(r.P, r.ny), NT, 0, S_, (const bf16_t *)g, (const bf16_t *)x, stat, ws, rows,
               C, r.G, r.GX, r.RL, r.rpb);
  CXN_LAUNCH((bn_ma_bwd_coef), (C + FC - 1) / FC, FL * FC, 0, S_, (const float *)ws, r.P, rows, C, stat, slope, gslope,
             gbias, coef);
  if (!dx) RET;
  const Geo a = make_geo(rows, C, vec, PMAX_APPLY);
  if (vec)
    CXN_LAUNCH((bn_ma_bwd_apply<8>), dim3(a.P, a.ny), NT, 0, S_, (const bf16_t *)g, (const bf16_t *)x, (bf16_t *)dx, stat,
               (const float *)coef, rows, C, a.G, a.GX, a.RL, a.rpb);
  else
    CXN_LAUNCH((bn_ma_bwd_apply<1>), dim3(a.P, a.ny), NT, 0, S_, (const bf16_t *)g, (const bf16_t *)x, (bf16_t *)dx, stat,
               (const float *)coef, rows, C, a.G, a.GX, a.RL, a.rpb);
  RET;
}
