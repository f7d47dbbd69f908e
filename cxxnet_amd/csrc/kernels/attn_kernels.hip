// attention: multi-head self-attention softmax(Q K^T / sqrt(d)) V over the tokens of an NHWC map
// (layers/extra.py AttentionLayer).  The input node is the fused qkv projection's output, rows
// [B T][3 C] bf16 with channel s C + h d + j = component j of head h of q / k / v (s = 0 / 1 / 2);
// the output is [B T][C].  d = 32 or 64, 1 <= T <= 1024.  Flash-style: no [T x T] matrix ever
// exists in global memory; the only state is the fp32 log-sum-exp (in natural units for the
// layer's state, and in the kernel's own log2 units for the backward) and the backward's row term
// D, [B nhead T] each.
//
//   cxn_attn_fwd   one launch: O and the log-sum-exp of every row
//   cxn_attn_bwd   two launches (three when dqkv aliases qkv): attn_bwd_dq over query tiles sweeps
//                  the keys twice (D = sum_j P dP first -- O is gone by then, so D cannot come from
//                  dO . O -- then dQ), attn_bwd_dkv over key tiles sweeps the queries for dK and dV
//
// Work split.  A block of 4 waves owns 64 rows (queries; keys in attn_bwd_dkv) of one (sample,
// head), a wave 16 of them, whose q (k, v) and dO fragments stay in registers.  The other side is
// streamed in chunks of 64 rows: two [64][d] tiles (K and V; Q and dO) per chunk, double buffered,
// fetched by 1-KiB LDS-DMAs straight from the strided rows -- head offset and q / k / v slice are
// in the descriptor's base, rows past T read zeros -- so chunk c + 1 lands under chunk c's MFMAs.
// 16-byte units of a tile row are XOR-swizzled with the row index (tile_addr): the row-major
// fragment reads (16 rows, one unit column) and the transposed reads both spread over the banks.
//
// Everything is computed transposed, so that no probability ever moves between lanes or through
// LDS.  S^T = K Q^T per 16 keys x 16 queries (16x16x32 MFMAs over d): lane (i, g) then holds query
// i and keys 4 g .. 4 g + 3 of the tile.  Softmax statistics are per-lane scalars (plus two
// shuffles over g): running max and sum in fp32, exp as v_exp_f32 of (s - m) log2e with 1 / sqrt(d)
// folded into the multiply, the O^T accumulators rescaled when the max moves.  Two S^T tiles of a
// lane are, as they stand, the B operand of O^T += V^T P^T over 32 keys in the key order
// (4 g + j, 16 + 4 g + j); the A operand V^T is read from the key-major V tile in the same order
// by ds_read_b64_tr_b16 pairs (tr_frag).  dQ^T, dK^T and dV^T are formed the same way.  P and dS
// are rounded to bf16 for those MFMAs; everything else is fp32 until the one rounding at the store.
//
// Hazards.  P and dS are VALU results feeding MFMA operands, which gfx950_prims.h's inline-asm
// MFMAs do not allow; every MFMA of this file is therefore the compiler builtin, for which hipcc
// inserts the wait states itself (the accumulators are short-lived or few, so the register
// shuffling that motivated the asm forms does not arise).  The LDS-DMAs are the asm form (dma16):
// completion is counted by hand, vmcnt(0) and a block barrier at the top of every chunk.
//
// Aliasing.  dqkv may be qkv.  attn_bwd_dkv reads its own K / V rows into registers before it
// stores over them and otherwise reads only q slices, so dK and dV go in place; dQ of the first
// launch then goes to a [B T][C] staging buffer and a third launch copies it onto the q slices
// after every reader of Q is done.  No atomics anywhere: the same bits on every run.
#include "attn_tile.h"

using namespace cxg;
using namespace cxg::attn;

namespace {

constexpr int NT = 256;
constexpr int RQ = 64;   // rows (queries or keys) a block owns, 16 per wave
constexpr int KC = 64;   // rows per streamed chunk

struct AttnArgs {
  int T, C, nhead, nt;  // tokens, channels of one of q / k / v, heads, row tiles per (sample, head)
  float sc2, scale;     // log2e / sqrt(d), 1 / sqrt(d)
};

struct Where {
  int lane, wave, i, g, tile, bh, b, h;
};
__device__ __forceinline__ Where where(const AttnArgs &a) {
  Where w;
  w.lane = threadIdx.x & 63;
  w.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  w.i = w.lane & 15;
  w.g = w.lane >> 4;
  w.tile = blockIdx.x % a.nt;
  w.bh = blockIdx.x / a.nt;
  w.b = w.bh / a.nhead;
  w.h = w.bh - w.b * a.nhead;
  return w;
}

// ------------------------------------------------------------------------------------ forward
template <int D>
__global__ __launch_bounds__(NT) void attn_fwd(const bf16_t *__restrict__ qkv, bf16_t *__restrict__ out,
                                               float *__restrict__ lse, float *__restrict__ lse2, const AttnArgs a) {
  constexpr int KS = D / 32, DT = D / 16, TILE = 64 * D * 2, BUF = 2 * TILE;
  __shared__ __attribute__((aligned(1024))) char smem[2 * BUF];
  const Where w = where(a);
  const int i = w.i, g = w.g, T = a.T;
  const size_t rs = 3 * static_cast<size_t>(a.C);
  const bf16_t *base = qkv + static_cast<size_t>(w.b) * T * rs + w.h * D;
  const uint32_t rsb = static_cast<uint32_t>(rs) * 2u, nrec = static_cast<uint32_t>(T - 1) * rsb + D * 2u;
  const rsrc_t rk = make_rsrc(base + a.C, nrec), rv = make_rsrc(base + 2 * a.C, nrec);
  const uint32_t lds0 = lds_base(smem);

  const int q = w.tile * RQ + w.wave * 16 + i;
  bf16x8 qf[KS];
  load_row<KS>(base + static_cast<size_t>(q < T ? q : 0) * rs, q < T, g, qf);

  float m = -INFINITY, l = 0.f;  // running max (log2 units) and this lane's share of the running sum
  f32x4 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nch = (T + KC - 1) / KC;
  stage2<D>(rk, rsb, rv, rsb, lds0, 0, T, w.wave, w.lane);
  for (int c = 0; c < nch; ++c) {
    wait_vmcnt<0>();
    __syncthreads();  // chunk c has landed; chunk c - 1's readers are done with the other buffer
    if (c + 1 < nch) stage2<D>(rk, rsb, rv, rsb, lds0 + ((c + 1) & 1) * BUF, (c + 1) * KC, T, w.wave, w.lane);
    const char *kb = smem + (c & 1) * BUF, *vb = kb + TILE;
    f32x4 s[4];
    float cm = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) s[kt] = mma(row_frag<D>(kb, 16 * kt + i, ks, g), qf[ks], s[kt]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s[kt][j] = c * KC + 16 * kt + 4 * g + j < T ? mul_rn(s[kt][j], a.sc2) : -INFINITY;
        cm = fmaxf(cm, s[kt][j]);
      }
    }
    cm = fmaxf(cm, __shfl_xor(cm, 16, 64));
    cm = fmaxf(cm, __shfl_xor(cm, 32, 64));  // finite: key c KC exists
    const float mn = fmaxf(m, cm);
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    m = mn;
    float ps = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s[kt][j] = __builtin_amdgcn_exp2f(s[kt][j] - mn);
        ps += s[kt][j];
      }
    l = l * alpha + ps;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int j = 0; j < 4; ++j) o[dt][j] *= alpha;
#pragma unroll
    for (int kp = 0; kp < 2; ++kp) {
      const bf16x8 pf = pack_frag(s[2 * kp], s[2 * kp + 1]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) o[dt] = mma(tr_frag<D>(vb, 32 * kp, dt, i, g), pf, o[dt]);
    }
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (q < T) {
    store_row<DT>(out + (static_cast<size_t>(w.b) * T + q) * a.C + w.h * D, g, o, 1.f / l);
    if (g == 0) {
      const float v = m + log2f(l);
      lse[static_cast<size_t>(w.bh) * T + q] = v * LN2;
      lse2[static_cast<size_t>(w.bh) * T + q] = v;
    }
  }
}

// ------------------------------------------------------------------- backward over query tiles
// Sweep 1 (it < nch): D_i = sum_j P_ij dP_ij into dsum.  Sweep 2: dQ = sum_j dS_ij K_j / sqrt(d)
// into dq (row stride dq_rs elements, the head's columns at h d).
template <int D>
__global__ __launch_bounds__(NT) void attn_bwd_dq(const bf16_t *__restrict__ qkv, const bf16_t *__restrict__ dout,
                                                  const float *__restrict__ lse2, float *__restrict__ dsum,
                                                  bf16_t *dq, long dq_rs, const AttnArgs a) {
  constexpr int KS = D / 32, DT = D / 16, TILE = 64 * D * 2, BUF = 2 * TILE;
  __shared__ __attribute__((aligned(1024))) char smem[2 * BUF];
  const Where w = where(a);
  const int i = w.i, g = w.g, T = a.T;
  const size_t rs = 3 * static_cast<size_t>(a.C);
  const bf16_t *base = qkv + static_cast<size_t>(w.b) * T * rs + w.h * D;
  const uint32_t rsb = static_cast<uint32_t>(rs) * 2u, nrec = static_cast<uint32_t>(T - 1) * rsb + D * 2u;
  const rsrc_t rk = make_rsrc(base + a.C, nrec), rv = make_rsrc(base + 2 * a.C, nrec);
  const uint32_t lds0 = lds_base(smem);

  const int q = w.tile * RQ + w.wave * 16 + i;
  const bool ok = q < T;
  const size_t row = static_cast<size_t>(w.b) * T + (ok ? q : 0);
  bf16x8 qf[KS], gf[KS];
  load_row<KS>(base + static_cast<size_t>(ok ? q : 0) * rs, ok, g, qf);
  load_row<KS>(dout + row * a.C + w.h * D, ok, g, gf);
  const float l2 = ok ? lse2[static_cast<size_t>(w.bh) * T + q] : 0.f;

  float dsl = 0.f, dv = 0.f;
  f32x4 acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nch = (T + KC - 1) / KC, nit = 2 * nch;
  stage2<D>(rk, rsb, rv, rsb, lds0, 0, T, w.wave, w.lane);
  for (int it = 0; it < nit; ++it) {
    const int c = it < nch ? it : it - nch;
    wait_vmcnt<0>();
    __syncthreads();
    if (it + 1 < nit) {
      const int cn = it + 1 < nch ? it + 1 : it + 1 - nch;
      stage2<D>(rk, rsb, rv, rsb, lds0 + ((it + 1) & 1) * BUF, cn * KC, T, w.wave, w.lane);
    }
    const char *kb = smem + (it & 1) * BUF, *vb = kb + TILE;
    f32x4 s[4], dp[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      s[kt] = dp[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        s[kt] = mma(row_frag<D>(kb, 16 * kt + i, ks, g), qf[ks], s[kt]);
        dp[kt] = mma(row_frag<D>(vb, 16 * kt + i, ks, g), gf[ks], dp[kt]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        s[kt][j] = c * KC + 16 * kt + 4 * g + j < T ? __builtin_amdgcn_exp2f(mul_rn(s[kt][j], a.sc2) - l2) : 0.f;
    }
    if (it < nch) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) dsl = fmaf(s[kt][j], dp[kt][j], dsl);
      if (it == nch - 1) {
        dsl += __shfl_xor(dsl, 16, 64);
        dsl += __shfl_xor(dsl, 32, 64);
        dv = dsl;
        if (ok && g == 0) dsum[static_cast<size_t>(w.bh) * T + q] = dv;
      }
    } else {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[kt][j] *= dp[kt][j] - dv;
#pragma unroll
      for (int kp = 0; kp < 2; ++kp) {
        const bf16x8 df = pack_frag(s[2 * kp], s[2 * kp + 1]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) acc[dt] = mma(tr_frag<D>(kb, 32 * kp, dt, i, g), df, acc[dt]);
      }
    }
  }
  if (ok) store_row<DT>(dq + row * dq_rs + w.h * D, g, acc, a.scale);
}

// --------------------------------------------------------------------- backward over key tiles
// dV = P^T dO and dK = dS^T Q / sqrt(d) of the wave's 16 keys over all queries, into the k and v
// slices of dqkv.  lse2 and D of a chunk's queries ride along in LDS.
template <int D>
__global__ __launch_bounds__(NT) void attn_bwd_dkv(const bf16_t *qkv, const bf16_t *__restrict__ dout,
                                                   const float *__restrict__ lse2, const float *__restrict__ dsum,
                                                   bf16_t *dqkv, const AttnArgs a) {
  constexpr int KS = D / 32, DT = D / 16, TILE = 64 * D * 2, BUF = 2 * TILE;
  __shared__ __attribute__((aligned(1024))) char smem[2 * BUF];
  __shared__ float stat[2][2][KC];  // [buffer][lse2 | D][query of the chunk]
  const Where w = where(a);
  const int i = w.i, g = w.g, T = a.T;
  const size_t rs = 3 * static_cast<size_t>(a.C);
  const bf16_t *base = qkv + static_cast<size_t>(w.b) * T * rs + w.h * D;
  const bf16_t *gbase = dout + static_cast<size_t>(w.b) * T * a.C + w.h * D;
  const uint32_t rsb = static_cast<uint32_t>(rs) * 2u, gsb = static_cast<uint32_t>(a.C) * 2u;
  const rsrc_t rq = make_rsrc(base, static_cast<uint32_t>(T - 1) * rsb + D * 2u);
  const rsrc_t rg = make_rsrc(gbase, static_cast<uint32_t>(T - 1) * gsb + D * 2u);
  const uint32_t lds0 = lds_base(smem);

  const int key = w.tile * RQ + w.wave * 16 + i;
  const bool ok = key < T;
  const size_t krow = static_cast<size_t>(ok ? key : 0) * rs;
  bf16x8 kf[KS], vf[KS];
  load_row<KS>(base + a.C + krow, ok, g, kf);
  load_row<KS>(base + 2 * a.C + krow, ok, g, vf);

  f32x4 dk[DT], dv[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dk[dt] = dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int tid = threadIdx.x, nch = (T + KC - 1) / KC;
  auto stage = [&](int c) __attribute__((always_inline)) {
    stage2<D>(rq, rsb, rg, gsb, lds0 + (c & 1) * BUF, c * KC, T, w.wave, w.lane);
    if (tid < 2 * KC) {  // a query past T: P = exp2(-inf) = 0 and dS = 0
      const int qq = c * KC + (tid & (KC - 1));
      const size_t e = static_cast<size_t>(w.bh) * T + (qq < T ? qq : 0);
      const float v = tid < KC ? lse2[e] : dsum[e];
      stat[c & 1][tid / KC][tid & (KC - 1)] = qq < T ? v : (tid < KC ? INFINITY : 0.f);
    }
  };
  stage(0);
  for (int c = 0; c < nch; ++c) {
    wait_vmcnt<0>();
    __syncthreads();
    if (c + 1 < nch) stage(c + 1);
    const char *qb = smem + (c & 1) * BUF, *gb = qb + TILE;
    f32x4 p[4], ds[4];
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      p[qt] = ds[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        p[qt] = mma(row_frag<D>(qb, 16 * qt + i, ks, g), kf[ks], p[qt]);
        ds[qt] = mma(row_frag<D>(gb, 16 * qt + i, ks, g), vf[ks], ds[qt]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ql = 16 * qt + 4 * g + j;
        p[qt][j] = __builtin_amdgcn_exp2f(mul_rn(p[qt][j], a.sc2) - stat[c & 1][0][ql]);
        ds[qt][j] = p[qt][j] * (ds[qt][j] - stat[c & 1][1][ql]);
      }
    }
#pragma unroll
    for (int qp = 0; qp < 2; ++qp) {
      const bf16x8 pf = pack_frag(p[2 * qp], p[2 * qp + 1]), df = pack_frag(ds[2 * qp], ds[2 * qp + 1]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        dv[dt] = mma(tr_frag<D>(gb, 32 * qp, dt, i, g), pf, dv[dt]);
        dk[dt] = mma(tr_frag<D>(qb, 32 * qp, dt, i, g), df, dk[dt]);
      }
    }
  }
  if (ok) {
    bf16_t *orow = dqkv + (static_cast<size_t>(w.b) * T + key) * rs + w.h * D;
    store_row<DT>(orow + a.C, g, dk, a.scale);
    store_row<DT>(orow + 2 * a.C, g, dv, 1.f);
  }
}

// dqkv[r][0 .. C) = stage[r][0 .. C), 16 bytes per lane
__global__ __launch_bounds__(NT) void attn_place_dq(const uint4 *__restrict__ stage, uint4 *dqkv, long rows, int cu) {
  const long n = rows * cu;
  for (long e = blockIdx.x * static_cast<long>(NT) + threadIdx.x; e < n; e += static_cast<long>(gridDim.x) * NT) {
    const long r = e / cu;
    dqkv[r * 3 * cu + (e - r * cu)] = stage[e];
  }
}

// head width, or 0 when the kernels do not serve the shape
static int head_dim(long B, long T, int C, int nhead) {
  if (B < 1 || T < 1 || T > 1024 || nhead < 1 || C < 1 || C > 65536 || C % nhead) return 0;  // (row offsets < 2^31)
  const int d = C / nhead;
  if (d != 32 && d != 64) return 0;
  if (B * nhead * ((T + RQ - 1) / RQ) > 0x7fffffffL) return 0;
  return d;
}

static AttnArgs make_args(int T, int C, int nhead, int d) {
  AttnArgs a;
  a.T = T;
  a.C = C;
  a.nhead = nhead;
  a.nt = (T + RQ - 1) / RQ;
  a.scale = d == 64 ? 0.125f : 0.17677669529663687f;
  a.sc2 = a.scale * LOG2E;
  return a;
}

}  // namespace

// Query (key) rows one block owns and keys (queries) per streamed chunk at head width d; -1: d not served.
CXN_API int cxn_attn_tile(int d, int *rows_per_block, int *keys_per_chunk) {
  if (d != 32 && d != 64) return -1;
  if (rows_per_block) *rows_per_block = RQ;
  if (keys_per_chunk) *keys_per_chunk = KC;
  return 0;
}

// out [B T][C] = softmax(q k^T / sqrt(d)) v per (sample, head) of qkv [B T][3 C]; lse [B nhead T] fp32
// receives every row's log-sum-exp and lse2 the same in log2 units, bit for bit the max + log2(sum)
// the kernel held -- what the backward subtracts, so that a row's recomputed P sums to the forward's 1
// (one key: P = 1 and dS = 0 exactly).  out must not alias qkv.
CXN_API int cxn_attn_fwd(const void *qkv, void *out, float *lse, float *lse2, int B, int T, int C, int nhead,
                         void *stream) {
  const int d = head_dim(B, T, C, nhead);
  if (!qkv || !out || !lse || !lse2 || qkv == out || !d || !(aligned16(qkv) && aligned16(out))) return -1;
  const AttnArgs a = make_args(T, C, nhead, d);
  const int grid = B * nhead * a.nt;
  const bf16_t *x = static_cast<const bf16_t *>(qkv);
  bf16_t *y = static_cast<bf16_t *>(out);
  if (d == 64) CXN_LAUNCH((attn_fwd<64>), grid, NT, 0, S_, x, y, lse, lse2, a);
  else CXN_LAUNCH((attn_fwd<32>), grid, NT, 0, S_, x, y, lse, lse2, a);
  RET;
}

// dqkv [B T][3 C] = the gradient of qkv given dout [B T][C] and the forward's lse2; dsum [B nhead T]
// fp32 is written (the row term D).  dqkv may be qkv: dq_stage, [B T][C] bf16, is then required
// (-2 without it) and receives dQ before a last launch places it; otherwise it is not touched.
CXN_API int cxn_attn_bwd(const void *qkv, const void *dout, const float *lse2, float *dsum, void *dqkv,
                         void *dq_stage, int B, int T, int C, int nhead, void *stream) {
  const int d = head_dim(B, T, C, nhead);
  if (!qkv || !dout || !lse2 || !dsum || !dqkv || !d || dout == dqkv ||
      !(aligned16(qkv) && aligned16(dout) && aligned16(dqkv)))
    return -1;
  const bool alias = qkv == dqkv;
  if (alias && !dq_stage) return -2;
  if (alias && !aligned16(dq_stage)) return -1;
  const AttnArgs a = make_args(T, C, nhead, d);
  const int grid = B * nhead * a.nt;
  const bf16_t *x = static_cast<const bf16_t *>(qkv), *g = static_cast<const bf16_t *>(dout);
  bf16_t *dx = static_cast<bf16_t *>(dqkv);
  bf16_t *dq = alias ? static_cast<bf16_t *>(dq_stage) : dx;
  const long dq_rs = alias ? C : 3L * C;
  if (d == 64) {
    CXN_LAUNCH((attn_bwd_dq<64>), grid, NT, 0, S_, x, g, lse2, dsum, dq, dq_rs, a);
    CXN_LAUNCH((attn_bwd_dkv<64>), grid, NT, 0, S_, x, g, lse2, (const float *)dsum, dx, a);
  } else {
    CXN_LAUNCH((attn_bwd_dq<32>), grid, NT, 0, S_, x, g, lse2, dsum, dq, dq_rs, a);
    CXN_LAUNCH((attn_bwd_dkv<32>), grid, NT, 0, S_, x, g, lse2, (const float *)dsum, dx, a);
  }
  if (alias) {
    const long rows = static_cast<long>(B) * T;
    CXN_LAUNCH((attn_place_dq), nblocks(rows * (C / 8)), NT, 0, S_, (const uint4 *)dq_stage, (uint4 *)dqkv, rows,
               C / 8);
  }
  RET;
}
