// Depthwise convolution (conv with ngroup = nchannel = the input channel count) as direct kernels:
// with one channel per group there is no reduction over channels and nothing for the MFMAs to
// do -- the layer is a K x K stencil per channel, bound by the bytes it moves.
//
//   cxn_dwconv_fwd         y  = [relu](dwconv(x, w) + bias)
//   cxn_dwconv_bwd_data    dx = dwconv_transpose(dy, w) [masked by relu'(z), dx = relu(z) on entry]
//   cxn_dwconv_bwd_weight  dw += sum over pixels of dy x;  db += sum of dy     (two launches)
//
// Served: groups == C == Cout (channel multiplier 1), C % 8 == 0, KH == KW in {3, 5}, stride in
// {1, 2}, pad_y and pad_x in [0, K) independently; everything else returns -1.  Activations are
// NHWC bf16 with an explicit pixel stride in elements (a node may be a channel slice of a wider
// buffer), weights [C][KH][KW][1] bf16, accumulation fp32.
//
// Geometry shared by the three kernels: a lane owns 8 consecutive channels (one 16-byte access)
// and keeps them for its whole walk, so its K K x 8 weights (and bias) are loaded once and stay
// in registers.  A block is GX group lanes x RL item lanes (GX = min(C / 8, 256), RL = 256 / GX),
// grid.y covers the groups beyond GX.  An item is a run of run_of(K) pixels along W of one row of the
// tensor the kernel writes (forward: y, data gradient: dx) or reduces over (weight gradient: dy):
// each row segment of the other operand is loaded once per item row and feeds every tap and every
// pixel of the run from registers.  A tap outside the image is a clamped address whose value is
// replaced by zero -- no padded copy of x, and no branch around a load, so all the loads of an item
// are in flight together.
//
// Weight gradient: pass 1, each block reduces its share of the items for its channels (lanes in
// registers, then the RL item lanes through LDS in a fixed order) into a slab of fp32 partials in
// the workspace; pass 2 merges the slabs in a fixed order (16 lanes per element over runs of
// consecutive slabs, then the lanes in lane order) and adds onto dw and db -- the scheme of
// bn_ma_kernels.hip.  No atomics: the same bits on every run.
#include "gfx950_prims.h"

namespace {

constexpr int NT = 256;
// pixels per item (even: the data gradient's column parity): 4 at 3 x 3; 2 at 5 x 5, whose 25 x 8
// weights leave registers for less.  The weight gradient takes 2 at both sizes: its K K x 8
// accumulators stay, and at 3 x 3 runs of 2 measured 1.1 - 1.5 times faster than runs of 4.
constexpr int run_of(int K) { return K == 3 ? 4 : 2; }
constexpr int wrun_of(int) { return 2; }
constexpr int PMAX = 512;     // weight gradient: slabs to aim for
constexpr int MIN_ITEMS = 4;  // and at least this many items per lane (amortises the block merge)
constexpr int GRID_CAP = 2048;

struct Dims {
  int N, H, W;    // the tensor the items walk (forward / weight gradient: the output side Ho, Wo)
  int Hs, Ws;     // the tensor the taps read (forward / weight gradient: x; data gradient: dy)
  int py, px, G, GX, RL;
  long ps_item, ps_src;  // pixel strides (elements) of the two
  uint32_t R, Wr, HWr;   // items, items per row, items per image
  FastDiv dWr, dHWr;
};

static bool make_dims(Dims &d, int N, int H, int W, int Hs, int Ws, int C, int py, int px, long ps_item, long ps_src,
                      int run) {
  d.N = N; d.H = H; d.W = W; d.Hs = Hs; d.Ws = Ws; d.py = py; d.px = px;
  d.G = C / 8;
  d.GX = d.G < NT ? d.G : NT;
  d.RL = NT / d.GX;
  d.ps_item = ps_item; d.ps_src = ps_src;
  const long wr = (W + run - 1) / run;
  const long r = static_cast<long>(N) * H * wr;
  if (r >= (1L << 31) - static_cast<long>(GRID_CAP) * NT) return false;  // (32-bit item walk)
  d.R = static_cast<uint32_t>(r);
  d.Wr = static_cast<uint32_t>(wr);
  d.HWr = static_cast<uint32_t>(H * wr);
  d.dWr = make_fastdiv(d.Wr);
  d.dHWr = make_fastdiv(d.HWr);
  return true;
}

struct Lane {
  int rl, grp;
  bool act;
};
__device__ __forceinline__ Lane lane_of(const Dims &d) {
  Lane l;
  const int t = threadIdx.x;
  l.rl = t / d.GX;
  l.grp = blockIdx.y * d.GX + (t - l.rl * d.GX);
  l.act = l.rl < d.RL && l.grp < d.G;
  return l;
}

__device__ __forceinline__ void item_of(const Dims &d, uint32_t r, int &n, int &h, int &wr) {
  const uint32_t nn = fdiv(r, d.dHWr);
  const uint32_t rem = r - nn * d.HWr;
  const uint32_t hh = fdiv(rem, d.dWr);
  n = static_cast<int>(nn);
  h = static_cast<int>(hh);
  wr = static_cast<int>(rem - hh * d.Wr);
}

// NL 16-byte loads of one image row at columns c0 .. c0 + NL - 1; a column outside [0, Wd), or
// any column of a row that is not there (rowok false; `row` then points at a clamped row), gives
// zeros: the address is clamped and the value selected
template <int NL>
__device__ __forceinline__ void load_cols(const bf16_t *row, long ps, int c0, int Wd, bool rowok, uint4 (&v)[NL]) {
#pragma unroll
  for (int m = 0; m < NL; ++m) {
    const int c = c0 + m;
    const bool ok = rowok && static_cast<unsigned>(c) < static_cast<unsigned>(Wd);
    const int cc = c < 0 ? 0 : (c >= Wd ? Wd - 1 : c);
    uint4 q = *reinterpret_cast<const uint4 *>(row + static_cast<size_t>(cc) * ps);
    q.x = ok ? q.x : 0u; q.y = ok ? q.y : 0u; q.z = ok ? q.z : 0u; q.w = ok ? q.w : 0u;
    v[m] = q;
  }
}

// The lane's 8 x KK weights ([C][KH][KW]: KK consecutive values per channel) as KK 16-byte loads,
// regrouped in registers to one packed 8-channel vector per tap
template <int KK>
__device__ __forceinline__ void load_weights(const bf16_t *w, int grp, uint4 (&wq)[KK]) {
  uint32_t raw[KK * 4];
  const uint4 *src = reinterpret_cast<const uint4 *>(w + static_cast<size_t>(grp) * 8 * KK);
#pragma unroll
  for (int i = 0; i < KK; ++i) {
    const uint4 q = src[i];
    raw[4 * i] = q.x; raw[4 * i + 1] = q.y; raw[4 * i + 2] = q.z; raw[4 * i + 3] = q.w;
  }
#pragma unroll
  for (int k = 0; k < KK; ++k) {
    uint32_t o[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int ia = (2 * jj) * KK + k, ib = (2 * jj + 1) * KK + k;
      const uint32_t a = (raw[ia >> 1] >> ((ia & 1) * 16)) & 0xffffu;
      const uint32_t b = (raw[ib >> 1] >> ((ib & 1) * 16)) & 0xffffu;
      o[jj] = a | (b << 16);
    }
    wq[k] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// ------------------------------------------------------------------------------------ forward
template <int K, int S>
__global__ __launch_bounds__(NT) void dwconv_fwd(const bf16_t *__restrict__ x, const bf16_t *__restrict__ w,
                                                 const float *__restrict__ bias, bf16_t *__restrict__ y, const Dims d,
                                                 int relu) {
  constexpr int RUN = run_of(K);
  constexpr int NL = (RUN - 1) * S + K;
  const Lane l = lane_of(d);
  if (!l.act) return;
  const size_t c0 = static_cast<size_t>(l.grp) * 8;
  uint4 wq[K * K];
  load_weights<K * K>(w, l.grp, wq);
  float bv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bv[j] = bias ? bias[c0 + j] : 0.f;
  const uint32_t step = gridDim.x * static_cast<uint32_t>(d.RL);
  for (uint32_t r = blockIdx.x * static_cast<uint32_t>(d.RL) + l.rl; r < d.R; r += step) {
    int n, ho, wr;
    item_of(d, r, n, ho, wr);
    const int wo0 = wr * RUN, wi0 = wo0 * S - d.px;
    float acc[RUN][8];
#pragma unroll
    for (int p = 0; p < RUN; ++p)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[p][j] = bv[j];
#pragma unroll
    for (int kh = 0; kh < K; ++kh) {
      const int hi = ho * S - d.py + kh;
      const bool rowok = static_cast<unsigned>(hi) < static_cast<unsigned>(d.Hs);
      const int hic = hi < 0 ? 0 : (hi >= d.Hs ? d.Hs - 1 : hi);
      const bf16_t *row = x + (static_cast<size_t>(n) * d.Hs + hic) * d.Ws * d.ps_src + c0;
      uint4 v[NL];
      load_cols<NL>(row, d.ps_src, wi0, d.Ws, rowok, v);
      float wf[K][8];
#pragma unroll
      for (int kw = 0; kw < K; ++kw) unpack8(wq[kh * K + kw], wf[kw]);
#pragma unroll
      for (int m = 0; m < NL; ++m) {
        float xf[8];
        unpack8(v[m], xf);
#pragma unroll
        for (int p = 0; p < RUN; ++p) {
          const int kw = m - p * S;
          if (kw >= 0 && kw < K) {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[p][j] = fmaf(xf[j], wf[kw][j], acc[p][j]);
          }
        }
      }
    }
    bf16_t *out = y + ((static_cast<size_t>(n) * d.H + ho) * d.W + wo0) * d.ps_item + c0;
#pragma unroll
    for (int p = 0; p < RUN; ++p) {
      if (wo0 + p < d.W) {
        if (relu) {
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[p][j] = fmaxf(acc[p][j], 0.f);
        }
        *reinterpret_cast<uint4 *>(out + static_cast<size_t>(p) * d.ps_item) = pack8(acc[p]);
      }
    }
  }
}

// ------------------------------------------------------------------------------ data gradient
// Gather form: dx[h][w] = sum over (kh, kw) of dy[(h + py - kh) / S][(w + px - kw) / S] w[kh][kw]
// over the taps whose two quotients are exact and inside dy.  Rows: every kh is tried and the ones
// that do not divide are zeroed like a border row.  Columns: a run starts at a multiple of the (even) run length and
// K - 1 is even, so the parity of the first column's numerator is PAR = px & 1 for the whole launch
// and the taps of each loaded dy column are known at compile time.
template <int K, int S, int PAR>
__global__ __launch_bounds__(NT) void dwconv_bwd_data(const bf16_t *__restrict__ dy, const bf16_t *__restrict__ w,
                                                      bf16_t *dx, const Dims d, int mask) {
  constexpr int RUN = run_of(K);
  constexpr int M = (RUN + K - 2 + PAR) / S + 1;
  const Lane l = lane_of(d);
  if (!l.act) return;
  const size_t c0 = static_cast<size_t>(l.grp) * 8;
  uint4 wq[K * K];
  load_weights<K * K>(w, l.grp, wq);
  const uint32_t step = gridDim.x * static_cast<uint32_t>(d.RL);
  for (uint32_t r = blockIdx.x * static_cast<uint32_t>(d.RL) + l.rl; r < d.R; r += step) {
    int n, h, wr;
    item_of(d, r, n, h, wr);
    const int w0 = wr * RUN;
    bf16_t *out = dx + ((static_cast<size_t>(n) * d.H + h) * d.W + w0) * d.ps_item + c0;
    uint4 prev[RUN];
    if (mask) {  // relu(z) of the node, read by the lane that overwrites it
#pragma unroll
      for (int p = 0; p < RUN; ++p) {
        const int pc = w0 + p < d.W ? p : 0;
        prev[p] = *reinterpret_cast<const uint4 *>(out + static_cast<size_t>(pc) * d.ps_item);
      }
    }
    const int b = w0 + d.px - (K - 1) - PAR;  // even at stride 2
    const int q0 = S == 1 ? b : b >> 1;
    float acc[RUN][8];
#pragma unroll
    for (int p = 0; p < RUN; ++p)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[p][j] = 0.f;
#pragma unroll
    for (int kh = 0; kh < K; ++kh) {
      const int t = h + d.py - kh;
      const int ho = S == 1 ? t : t >> 1;
      const bool rowok = t >= 0 && (S == 1 || (t & 1) == 0) && ho < d.Hs;
      const int hoc = ho < 0 ? 0 : (ho >= d.Hs ? d.Hs - 1 : ho);
      const bf16_t *row = dy + (static_cast<size_t>(n) * d.Hs + hoc) * d.Ws * d.ps_src + c0;
      uint4 v[M];
      load_cols<M>(row, d.ps_src, q0, d.Ws, rowok, v);
      float wf[K][8];
#pragma unroll
      for (int kw = 0; kw < K; ++kw) unpack8(wq[kh * K + kw], wf[kw]);
#pragma unroll
      for (int m = 0; m < M; ++m) {
        float gf[8];
        unpack8(v[m], gf);
#pragma unroll
        for (int p = 0; p < RUN; ++p) {
          const int kw = p + K - 1 + PAR - m * S;
          if (kw >= 0 && kw < K) {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[p][j] = fmaf(gf[j], wf[kw][j], acc[p][j]);
          }
        }
      }
    }
#pragma unroll
    for (int p = 0; p < RUN; ++p) {
      if (w0 + p < d.W) {
        if (mask) {
          float zf[8];
          unpack8(prev[p], zf);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[p][j] = zf[j] > 0.f ? acc[p][j] : 0.f;
        }
        *reinterpret_cast<uint4 *>(out + static_cast<size_t>(p) * d.ps_item) = pack8(acc[p]);
      }
    }
  }
}

// ---------------------------------------------------------------------------- weight gradient
// slab p of ws: [C][K K] partial dw, then [C] partial db, of items [p ipb, min(R, (p + 1) ipb))
template <int K, int S>
__global__ __launch_bounds__(NT) void dwconv_wgrad_partial(const bf16_t *__restrict__ x, const bf16_t *__restrict__ dy,
                                                           float *__restrict__ ws, const Dims d, uint32_t ipb, int C) {
  constexpr int RW = wrun_of(K);
  constexpr int NL = (RW - 1) * S + K;
  constexpr int KK = K * K;
  __shared__ float s_red[NT * 8];
  const Lane l = lane_of(d);
  const size_t c0 = static_cast<size_t>(l.grp) * 8;
  float acc[KK][8], accb[8];
#pragma unroll
  for (int k = 0; k < KK; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) accb[j] = 0.f;
  if (l.act) {
    const uint32_t r0 = blockIdx.x * ipb;
    const uint32_t r1 = r0 + ipb < d.R ? r0 + ipb : d.R;
    for (uint32_t r = r0 + l.rl; r < r1; r += static_cast<uint32_t>(d.RL)) {
      int n, ho, wr;
      item_of(d, r, n, ho, wr);
      const int wo0 = wr * RW, wi0 = wo0 * S - d.px;
      uint4 gq[RW];
      load_cols<RW>(dy + (static_cast<size_t>(n) * d.H + ho) * d.W * d.ps_item + c0, d.ps_item, wo0, d.W, true, gq);
      float gf[RW][8];
#pragma unroll
      for (int p = 0; p < RW; ++p) {
        unpack8(gq[p], gf[p]);
#pragma unroll
        for (int j = 0; j < 8; ++j) accb[j] += gf[p][j];
      }
#pragma unroll
      for (int kh = 0; kh < K; ++kh) {
        const int hi = ho * S - d.py + kh;
        const bool rowok = static_cast<unsigned>(hi) < static_cast<unsigned>(d.Hs);
        const int hic = hi < 0 ? 0 : (hi >= d.Hs ? d.Hs - 1 : hi);
        const bf16_t *row = x + (static_cast<size_t>(n) * d.Hs + hic) * d.Ws * d.ps_src + c0;
        uint4 v[NL];
        load_cols<NL>(row, d.ps_src, wi0, d.Ws, rowok, v);
#pragma unroll
        for (int m = 0; m < NL; ++m) {
          float xf[8];
          unpack8(v[m], xf);
#pragma unroll
          for (int p = 0; p < RW; ++p) {
            const int kw = m - p * S;
            if (kw >= 0 && kw < K) {
#pragma unroll
              for (int j = 0; j < 8; ++j) acc[kh * K + kw][j] = fmaf(gf[p][j], xf[j], acc[kh * K + kw][j]);
            }
          }
        }
      }
    }
  }
  // the RL item lanes of each group, summed in lane order: one round per tap, the last one for db
  const int t = threadIdx.x;
  float *slab = ws + static_cast<size_t>(blockIdx.x) * C * (KK + 1);
#pragma unroll
  for (int k = 0; k <= KK; ++k) {
    const float *a = k < KK ? acc[k % KK] : accb;
    *reinterpret_cast<float4 *>(&s_red[t * 8]) = make_float4(a[0], a[1], a[2], a[3]);
    *reinterpret_cast<float4 *>(&s_red[t * 8 + 4]) = make_float4(a[4], a[5], a[6], a[7]);
    __syncthreads();
    for (int q = t; q < d.GX * 8; q += NT) {
      const int grp = blockIdx.y * d.GX + (q >> 3);
      float sum = 0.f;
      for (int rl = 0; rl < d.RL; ++rl) sum += s_red[rl * d.GX * 8 + q];
      if (grp < d.G) {
        const size_t c = static_cast<size_t>(grp) * 8 + (q & 7);
        slab[k < KK ? c * KK + k : static_cast<size_t>(C) * KK + c] = sum;
      }
    }
    __syncthreads();
  }
}

// dw[e] += sum over the slabs; e past nw: db.  ML lanes per element each sum a run of consecutive
// slabs in slab order, lane 0 then sums the lanes in lane order: a fixed order, and P / ML dependent
// loads per lane instead of P (one lane per element ran the 3 x 3 x 32-channel layer's 512 slabs
// in 60 us, most of the weight gradient's time)
constexpr int ML = 16, MC = NT / ML;
__global__ __launch_bounds__(NT) void dwconv_wgrad_merge(const float *__restrict__ ws, int P, long slab, float *dw,
                                                         float *db, int nw, int C) {
  __shared__ float s_sum[ML][MC];
  const int el = threadIdx.x % MC, ln = threadIdx.x / MC;
  const int e = blockIdx.x * MC + el;
  const int ne = nw + (db ? C : 0);
  const int chunk = (P + ML - 1) / ML;
  const int p0 = ln * chunk, p1 = p0 + chunk < P ? p0 + chunk : P;
  float sum = 0.f;
  if (e < ne) {
#pragma unroll 8
    for (int p = p0; p < p1; ++p) sum += ws[static_cast<size_t>(p) * slab + e];
  }
  s_sum[ln][el] = sum;
  __syncthreads();
  if (ln != 0 || e >= ne) return;
  for (int q = 1; q < ML; ++q) sum += s_sum[q][el];
  if (e < nw) dw[e] += sum;
  else db[e - nw] += sum;
}

// what the kernels serve; Ho / Wo by the layer's rule
static bool serves(int N, int H, int W, int C, int Cout, int groups, int KH, int KW, int stride, int pad_y, int pad_x,
                   int &Ho, int &Wo) {
  if (N < 1 || H < 1 || W < 1 || C < 8 || C % 8 || groups != C || Cout != C) return false;
  if (KH != KW || (KH != 3 && KH != 5) || (stride != 1 && stride != 2)) return false;
  if (pad_y < 0 || pad_y >= KH || pad_x < 0 || pad_x >= KW) return false;
  if (H + 2 * pad_y < KH || W + 2 * pad_x < KW) return false;
  Ho = (H + 2 * pad_y - KH) / stride + 1;
  Wo = (W + 2 * pad_x - KW) / stride + 1;
  return true;
}

static dim3 walk_grid(const Dims &d) {
  const int ny = (d.G + d.GX - 1) / d.GX;
  long nb = (static_cast<long>(d.R) + d.RL - 1) / d.RL;
  const long cap = GRID_CAP / ny > 1 ? GRID_CAP / ny : 1;
  nb = nb < 1 ? 1 : (nb > cap ? cap : nb);
  return dim3(static_cast<unsigned>(nb), static_cast<unsigned>(ny));
}

}  // namespace


// y = [relu](dwconv(x, w) + bias); xs / ys: pixel strides in elements; bias nullable.
CXN_API int cxn_dwconv_fwd(const void *x, long xs, const void *w, const float *bias, void *y, long ys, int N, int H,
                           int W, int C, int Cout, int groups, int KH, int KW, int stride, int pad_y, int pad_x,
                           int relu, void *stream) {
  int Ho, Wo;
  if (!serves(N, H, W, C, Cout, groups, KH, KW, stride, pad_y, pad_x, Ho, Wo)) return -1;
  if (xs < C || ys < C || xs % 8 || ys % 8 || !aligned16(x) || !aligned16(y) || !aligned16(w)) return -1;
  Dims d;
  if (!make_dims(d, N, Ho, Wo, H, W, C, pad_y, pad_x, ys, xs, run_of(KH))) return -1;
  const dim3 grid = walk_grid(d);
#define CXN_DW_FWD(K_, ST_)                                                                                         \
  CXN_LAUNCH((dwconv_fwd<K_, ST_>), grid, NT, 0, S_, (const bf16_t *)x, (const bf16_t *)w, bias, (bf16_t *)y, d, relu)
  if (KH == 3) {
    if (stride == 1) CXN_DW_FWD(3, 1);
    else CXN_DW_FWD(3, 2);
  } else {
    if (stride == 1) CXN_DW_FWD(5, 1);
    else CXN_DW_FWD(5, 2);
  }
#undef CXN_DW_FWD
  RET;
}

// dx [N][H][W][C] = dwconv_transpose(dy, w), every element written; H, W: the forward input size
// (at stride 2 several give the same Ho, Wo).  mask_relu: dx holds relu(z) on entry and the result
// is exactly 0 where that is not > 0.
CXN_API int cxn_dwconv_bwd_data(const void *dy, long dys, const void *w, void *dx, long dxs, int N, int H, int W,
                                int C, int Cout, int groups, int KH, int KW, int stride, int pad_y, int pad_x,
                                int mask_relu, void *stream) {
  int Ho, Wo;
  if (!serves(N, H, W, C, Cout, groups, KH, KW, stride, pad_y, pad_x, Ho, Wo)) return -1;
  if (dys < C || dxs < C || dys % 8 || dxs % 8 || !aligned16(dy) || !aligned16(dx) || !aligned16(w)) return -1;
  Dims d;
  if (!make_dims(d, N, H, W, Ho, Wo, C, pad_y, pad_x, dxs, dys, run_of(KH))) return -1;
  const dim3 grid = walk_grid(d);
  const int par = stride == 2 ? (pad_x & 1) : 0;
#define CXN_DW_BD(K_, ST_, PAR_)                                                                                    \
  CXN_LAUNCH((dwconv_bwd_data<K_, ST_, PAR_>), grid, NT, 0, S_, (const bf16_t *)dy, (const bf16_t *)w, (bf16_t *)dx, d, \
             mask_relu)
  if (KH == 3) {
    if (stride == 1) CXN_DW_BD(3, 1, 0);
    else if (par == 0) CXN_DW_BD(3, 2, 0);
    else CXN_DW_BD(3, 2, 1);
  } else {
    if (stride == 1) CXN_DW_BD(5, 1, 0);
    else if (par == 0) CXN_DW_BD(5, 2, 0);
    else CXN_DW_BD(5, 2, 1);
  }
#undef CXN_DW_BD
  RET;
}

// dw [C][KH][KW] += sum over pixels of dy x; db [C] (nullable) += sum of dy.  ws: fp32 workspace of
// ws_floats >= P C (K K + 1), P the slab count below (mirrored by ops.gemm.dwconv_wgrad_partials);
// -2 when it is smaller.
CXN_API int cxn_dwconv_bwd_weight(const void *x, long xs, const void *dy, long dys, float *dw, float *db, float *ws,
                                  long ws_floats, int N, int H, int W, int C, int Cout, int groups, int KH, int KW,
                                  int stride, int pad_y, int pad_x, void *stream) {
  int Ho, Wo;
  if (!serves(N, H, W, C, Cout, groups, KH, KW, stride, pad_y, pad_x, Ho, Wo)) return -1;
  if (xs < C || dys < C || xs % 8 || dys % 8 || !aligned16(x) || !aligned16(dy)) return -1;
  Dims d;
  if (!make_dims(d, N, Ho, Wo, H, W, C, pad_y, pad_x, dys, xs, wrun_of(KH))) return -1;
  const int ny = (d.G + d.GX - 1) / d.GX;
  const long pmax = PMAX / ny > 1 ? PMAX / ny : 1;
  const long floor_ipb = static_cast<long>(d.RL) * MIN_ITEMS;
  const long even = (static_cast<long>(d.R) + pmax - 1) / pmax;
  const long ipb = even > floor_ipb ? even : floor_ipb;
  const int P = static_cast<int>((static_cast<long>(d.R) + ipb - 1) / ipb);
  const long slab = static_cast<long>(C) * (KH * KW + 1);
  if (!ws || static_cast<long>(P) * slab > ws_floats) return -2;
  const dim3 grid(static_cast<unsigned>(P), static_cast<unsigned>(ny));
#define CXN_DW_WG(K_, ST_)                                                                                          \
  CXN_LAUNCH((dwconv_wgrad_partial<K_, ST_>), grid, NT, 0, S_, (const bf16_t *)x, (const bf16_t *)dy, ws, d,         \
             static_cast<uint32_t>(ipb), C)
  if (KH == 3) {
    if (stride == 1) CXN_DW_WG(3, 1);
    else CXN_DW_WG(3, 2);
  } else {
    if (stride == 1) CXN_DW_WG(5, 1);
    else CXN_DW_WG(5, 2);
  }
#undef CXN_DW_WG
  const int nw = C * KH * KW;
  CXN_LAUNCH((dwconv_wgrad_merge), (nw + C + MC - 1) / MC, NT, 0, S_, (const float *)ws, P, slab, dw, db, nw, C);
  RET;
}
