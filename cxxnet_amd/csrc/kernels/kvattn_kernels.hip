// kv_attention: multi-head attention of many queries over a short key / value set (layers/extra.py
// KVAttentionLayer) -- the spatial-reduction attention of the pyramid transformers, where the
// queries are every position of a map (Tq up to 16384) and the keys and values come from a reduced
// copy of it (Tk <= 64).  q is [B Tq][C] bf16, channel h d + j = component j of head h; kv is
// [B Tk][2 C], channel s C + h d + j with s = 0 for k and 1 for v; the output is [B Tq][C];
// d = 32 or 64.  The forward leaves the fp32 log-sum-exp of every query row, [B nhead Tq], for the
// layer; the backward reads no state (below).
//
//   cxn_kvattn_fwd   one launch: O and the log-sum-exp of every row
//   cxn_kvattn_bwd   one launch for dQ and the block's share of dK, dV; with more than one split
//                    of the queries a second launch merges the fp32 slabs in a fixed order
//
// Resident K / V.  The whole key set of a (sample, head) is one [64][d] tile each of K and V (the
// swizzled tile of attn_tile.h), staged once per block by LDS-DMA from the strided kv rows -- head
// offset and k / v slice in the descriptor base, rows >= Tk arrive as zeros -- and kept while the
// block walks a run of 64-query tiles, a wave 16 queries of each.  With every key present there is
// no running max and no rescale: a query's <= 64 logits sit in the registers of its lane group
// (lane (i, g) holds query i and keys 16 kt + 4 g + j), the softmax is max, then exp2 and sum, with
// two shuffles over g each, and keys >= Tk take probability exactly 0 by a select, not by their
// zero rows.  Products are computed transposed as in attn_kernels.hip (S^T = K Q^T), so P^T is the
// B operand of O^T += V^T P^T as it stands; the logit is mul_rn(q.k, log2e / sqrt(d)).
//
// No lse2.  attention's backward forms P = exp2(logit - lse2) from a stored max + log2(sum).  With
// every key in registers the backward here runs the two-step softmax again instead,
// P = exp2(logit - max) (1 / sum): the rows then sum to 1 within a few fp32 ulps of 1, where
// subtracting a rounded lse2 leaves them off by ulp(lse2), about 4e-6 at a logit of 36.  That
// matters in a row one key dominates: D = sum_j P dP then carries (sum P - 1) dP of that key and
// its dS = P (dP - D) no longer cancels.  Measured on such a row (Tk = 17, a key of four times the
// usual norm): 1.11 of the test's bound with lse2, inside it without; and a state array and its
// loads are gone.  Both orientations read the same max and 1 / sum, so they form the same P bits.
//
// Forward.  Q fragments go from global memory straight to registers, the next tile's under the
// current tile's MFMAs; nothing but K / V is in LDS.  Grid (sample, split of FWD_RUN tiles, head),
// head fastest: the heads of one run of rows run adjacent and together read whole q rows.
//
// Backward -- where this file leaves the plan of one [64 keys][d] fp32 accumulator pair per wave.
// dQ^T = K^T dS^T contracts over the keys, which the transposed orientation serves from registers;
// dK^T = Q^T dS and dV^T = dO^T P contract over the queries, and an MFMA operand must then hold
// several queries of one key in a lane: the other orientation.  Turning P and dS through LDS costs
// two [64][64] bf16 writes and transposed reads per tile, and leaves every wave with all 64 keys:
// 2 x [64][d] fp32 = 128 accumulator registers per lane at d = 64, and a four-way sum through LDS
// at the end.  Instead the tile's logits and dP are recomputed in the key orientation (wave w owns
// keys 16 w .. 16 w + 15 against the tile's 64 queries, as attn_bwd_dkv does): 16 more MFMAs per
// wave and tile at d = 64 on top of 40, in a kernel whose tile moves 24 KiB of HBM traffic per
// ~0.8 us of MFMA time, and in exchange
//   - the accumulators are the wave's own 16 keys: 2 x [16][d] fp32 = 32 registers at d = 64, no
//     spill risk, no d-split and no cross-wave sum: each wave stores its rows of the slab itself;
//   - waves whose 16 keys are all >= Tk skip that half.
// The key orientation needs Q^T and dO^T as transposed operands, which only ds_read_b64_tr_b16
// provides, so in the backward the Q and dO tiles do pass through LDS: one DMA staging per tile,
// double buffered (tile t + 1 lands under tile t's MFMAs), and the query orientation reads its
// fragments from the same tiles, so q and dO are still fetched from memory exactly once.  The row
// terms max, 1 / sum and D = sum_j P dP (register sums plus two shuffles each, no second sweep, no
// dsum state) ride in LDS between the two orientations.  LDS: (2 + 4) tiles = 48 KiB at d = 64, 24 KiB at 32.
//
// Work split of the backward.  Grid (sample, split, head).  A (sample, head)'s nt = ceil(Tq / 64)
// query tiles are cut into splits = ceil(nt / BWD_RUN) runs of equal length: a function of Tq
// alone, never of B, so a sample's gradient does not change with the batch it is in.  BWD_RUN = 4
// keeps a block's fp32 slab [2][Tk][d] (at most 32 KiB) under a third of what its run reads and
// writes (4 x 24 KiB), and gives PVTv2's first stage (Tq = 3136, one head) 13 blocks per sample
// where attn_bwd_dkv had one.  With one split the block rounds and stores dK, dV itself;
// otherwise kvattn_merge adds the slabs of a (sample, head) in split order, scales dK, rounds once
// and writes the k and v slices of dkv.  No atomics: two runs give the same bits.
//
// Aliasing.  dq may be q: a tile's q rows are in LDS (vmcnt(0) + block barrier) before any wave
// stores dQ over them, the DMAs in flight meanwhile fetch the next tile's rows, and no other block
// reads those columns of those rows.  dkv may be kv: dK / dV reach dkv in the merge, after every
// block has finished, or with one split at the end of the only block that ever reads that head's
// k / v columns of that sample, long after it staged them.
//
// Hazards.  P and dS are VALU results feeding MFMA operands: every MFMA is the compiler builtin
// (see attn_kernels.hip).  The DMAs are the asm form; completion is vmcnt(0) plus a block barrier.
#include "attn_tile.h"

using namespace cxg;
using namespace cxg::attn;

namespace {

constexpr int NT = 256;
constexpr int TQ = 64;       // queries per tile, 16 per wave
constexpr int TK = 64;       // keys at most
constexpr int FWD_RUN = 4;   // query tiles a forward block walks
constexpr int BWD_RUN = 4;   // query tiles a backward block walks at most

struct KVArgs {
  int Tq, Tk, C, nhead;  // queries, keys, channels of q (kv has 2 C), heads
  int nt, fsplits, per, splits;  // query tiles; forward runs; backward: tiles per run, runs
  float sc2, scale;      // log2e / sqrt(d), 1 / sqrt(d)
};

struct Where {
  int lane, wave, i, g, b, h, split;
};
__device__ __forceinline__ Where where(int nhead, int splits) {
  Where w;
  w.lane = threadIdx.x & 63;
  w.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  w.i = w.lane & 15;
  w.g = w.lane >> 4;
  w.h = blockIdx.x % nhead;
  const int rest = blockIdx.x / nhead;
  w.split = rest % splits;
  w.b = rest / splits;
  return w;
}

// ------------------------------------------------------------------------------------ forward
template <int D>
__global__ __launch_bounds__(NT) void kvattn_fwd(const bf16_t *__restrict__ q, const bf16_t *__restrict__ kv,
                                                 bf16_t *__restrict__ out, float *__restrict__ lse,
                                                 const KVArgs a) {
  constexpr int KS = D / 32, DT = D / 16, TILE = 64 * D * 2;
  __shared__ __attribute__((aligned(1024))) char smem[2 * TILE];  // K | V
  const Where w = where(a.nhead, a.fsplits);
  const int i = w.i, g = w.g, Tq = a.Tq, Tk = a.Tk;
  const size_t C = static_cast<size_t>(a.C);
  const bf16_t *kbase = kv + static_cast<size_t>(w.b) * Tk * 2 * C + w.h * D;
  const uint32_t ksb = static_cast<uint32_t>(C) * 4u, krec = static_cast<uint32_t>(Tk - 1) * ksb + D * 2u;
  stage2<D>(make_rsrc(kbase, krec), ksb, make_rsrc(kbase + C, krec), ksb, lds_base(smem), 0, Tk, w.wave, w.lane);

  const bf16_t *qbase = q + static_cast<size_t>(w.b) * Tq * C + w.h * D;
  bf16_t *obase = out + static_cast<size_t>(w.b) * Tq * C + w.h * D;
  const size_t sbase = (static_cast<size_t>(w.b) * a.nhead + w.h) * Tq;
  const int t0 = w.split * FWD_RUN, t1 = t0 + FWD_RUN < a.nt ? t0 + FWD_RUN : a.nt;
  bf16x8 qn[KS];
  {
    const int qq = t0 * TQ + w.wave * 16 + i;
    load_row<KS>(qbase + static_cast<size_t>(qq < Tq ? qq : 0) * C, qq < Tq, g, qn);
  }
  wait_vmcnt<0>();
  __syncthreads();  // K and V are resident; no barrier follows
  const char *kb = smem, *vb = smem + TILE;

  for (int t = t0; t < t1; ++t) {
    const int qi = t * TQ + w.wave * 16 + i;
    bf16x8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = qn[ks];
    if (t + 1 < t1) {
      const int qq = qi + TQ;
      load_row<KS>(qbase + static_cast<size_t>(qq < Tq ? qq : 0) * C, qq < Tq, g, qn);
    }
    f32x4 s[4];
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) s[kt] = mma(row_frag<D>(kb, 16 * kt + i, ks, g), qf[ks], s[kt]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s[kt][j] = 16 * kt + 4 * g + j < Tk ? mul_rn(s[kt][j], a.sc2) : -INFINITY;
        m = fmaxf(m, s[kt][j]);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));  // finite: key 0 exists
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s[kt][j] = __builtin_amdgcn_exp2f(s[kt][j] - m);
        l += s[kt][j];
      }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kp = 0; kp < 2; ++kp) {
      const bf16x8 pf = pack_frag(s[2 * kp], s[2 * kp + 1]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) o[dt] = mma(tr_frag<D>(vb, 32 * kp, dt, i, g), pf, o[dt]);
    }
    if (qi < Tq) {
      store_row<DT>(obase + static_cast<size_t>(qi) * C, g, o, 1.f / l);
      if (g == 0) lse[sbase + qi] = (m + log2f(l)) * LN2;
    }
  }
}

// ------------------------------------------------------------------------------------ backward
// Block (sample, split, head) walks query tiles split per .. of its head.  dkv non-null (one
// split): dK / dV are rounded and stored; else the block's fp32 slab [2][Tk][D] is.
template <int D>
__global__ __launch_bounds__(NT) void kvattn_bwd(const bf16_t *q, const bf16_t *kv, const bf16_t *__restrict__ dout,
                                                 bf16_t *dq, bf16_t *dkv, float *__restrict__ slabs,
                                                 const KVArgs a) {
  constexpr int KS = D / 32, DT = D / 16, TILE = 64 * D * 2, BUF = 2 * TILE;
  __shared__ __attribute__((aligned(1024))) char smem[BUF + 2 * BUF];  // K | V | 2 x (Q | dO)
  __shared__ float stat[3][TQ];                                        // [max | 1 / sum | D][query of the tile]
  const Where w = where(a.nhead, a.splits);
  const int i = w.i, g = w.g, Tq = a.Tq, Tk = a.Tk, tid = threadIdx.x;
  const size_t C = static_cast<size_t>(a.C);
  const bf16_t *kbase = kv + static_cast<size_t>(w.b) * Tk * 2 * C + w.h * D;
  const size_t qoff = static_cast<size_t>(w.b) * Tq * C + w.h * D;
  const uint32_t ksb = static_cast<uint32_t>(C) * 4u, krec = static_cast<uint32_t>(Tk - 1) * ksb + D * 2u;
  const uint32_t qsb = static_cast<uint32_t>(C) * 2u, qrec = static_cast<uint32_t>(Tq - 1) * qsb + D * 2u;
  const rsrc_t rq = make_rsrc(q + qoff, qrec), rg = make_rsrc(dout + qoff, qrec);
  const uint32_t lds0 = lds_base(smem);
  const int t0 = w.split * a.per, n = t0 + a.per < a.nt ? a.per : a.nt - t0;

  // tile t0 + c into buffer c & 1; the q and dO rows of a query past Tq arrive as zeros
  auto stage = [&](int c) __attribute__((always_inline)) {
    stage2<D>(rq, qsb, rg, qsb, lds0 + BUF + (c & 1) * BUF, (t0 + c) * TQ, Tq, w.wave, w.lane);
  };
  stage2<D>(make_rsrc(kbase, krec), ksb, make_rsrc(kbase + C, krec), ksb, lds0, 0, Tk, w.wave, w.lane);
  stage(0);
  wait_vmcnt<0>();
  __syncthreads();  // K and V are resident

  const char *kb = smem, *vb = smem + TILE;
  const int key = w.wave * 16 + i;  // key orientation: the wave's 16 keys
  const bool busy = w.wave * 16 < Tk, okk = key < Tk;
  bf16x8 kf[KS], vf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    kf[ks] = row_frag<D>(kb, key, ks, g);
    vf[ks] = row_frag<D>(vb, key, ks, g);
  }
  f32x4 dk[DT], dv[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dk[dt] = dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int c = 0; c < n; ++c) {
    wait_vmcnt<0>();
    __syncthreads();  // tile c is in LDS (dQ may now go over its q rows); tile c - 1's readers are done
    if (c + 1 < n) stage(c + 1);
    const char *qb = smem + BUF + (c & 1) * BUF, *gb = qb + TILE;
    float *st = &stat[0][0];
    {  // query orientation: the wave's 16 queries against all keys -- D, dS, dQ
      const int tq = w.wave * 16 + i, qi = (t0 + c) * TQ + tq;
      bf16x8 qf[KS], gf[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        qf[ks] = row_frag<D>(qb, tq, ks, g);
        gf[ks] = row_frag<D>(gb, tq, ks, g);
      }
      f32x4 p[4], dp[4];
      float m = -INFINITY, l = 0.f, dsl = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        p[kt] = dp[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          p[kt] = mma(row_frag<D>(kb, 16 * kt + i, ks, g), qf[ks], p[kt]);
          dp[kt] = mma(row_frag<D>(vb, 16 * kt + i, ks, g), gf[ks], dp[kt]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          p[kt][j] = 16 * kt + 4 * g + j < Tk ? mul_rn(p[kt][j], a.sc2) : -INFINITY;
          m = fmaxf(m, p[kt][j]);
        }
      }
      m = fmaxf(m, __shfl_xor(m, 16, 64));
      m = fmaxf(m, __shfl_xor(m, 32, 64));  // finite: key 0 exists
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          p[kt][j] = __builtin_amdgcn_exp2f(p[kt][j] - m);
          l += p[kt][j];
        }
      l += __shfl_xor(l, 16, 64);
      l += __shfl_xor(l, 32, 64);
      const float il = qi < Tq ? 1.f / l : 0.f;  // a query past Tq: P = 0
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          p[kt][j] *= il;
          dsl = fmaf(p[kt][j], dp[kt][j], dsl);
        }
      dsl += __shfl_xor(dsl, 16, 64);
      dsl += __shfl_xor(dsl, 32, 64);
      if (g == 0) st[tq] = m, st[TQ + tq] = il, st[2 * TQ + tq] = dsl;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) p[kt][j] *= dp[kt][j] - dsl;  // dS
      f32x4 acc[DT];
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kp = 0; kp < 2; ++kp) {
        const bf16x8 df = pack_frag(p[2 * kp], p[2 * kp + 1]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) acc[dt] = mma(tr_frag<D>(kb, 32 * kp, dt, i, g), df, acc[dt]);
      }
      if (qi < Tq) store_row<DT>(dq + qoff + static_cast<size_t>(qi) * C, g, acc, a.scale);
    }
    __syncthreads();  // the row terms of the tile's 64 queries are in LDS
    if (busy) {       // key orientation: the wave's 16 keys against the tile's queries -- dK, dV
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
          p[qt][j] = okk ? __builtin_amdgcn_exp2f(mul_rn(p[qt][j], a.sc2) - st[ql]) * st[TQ + ql] : 0.f;
          ds[qt][j] = p[qt][j] * (ds[qt][j] - st[2 * TQ + ql]);
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
  }
  if (!okk) return;
  if (dkv) {
    bf16_t *orow = dkv + (static_cast<size_t>(w.b) * Tk + key) * 2 * C + w.h * D;
    store_row<DT>(orow, g, dk, a.scale);
    store_row<DT>(orow + C, g, dv, 1.f);
  } else {
    float *slab = slabs + ((static_cast<size_t>(w.b) * a.nhead + w.h) * a.splits + w.split) * 2 * Tk * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      *reinterpret_cast<f32x4 *>(slab + key * D + 16 * dt + 4 * g) = dk[dt];
      *reinterpret_cast<f32x4 *>(slab + (Tk + key) * D + 16 * dt + 4 * g) = dv[dt];
    }
  }
}

// dkv's k and v slices = the sum over the splits, in split order, of slab (sample, head, split),
// dK scaled by 1 / sqrt(d), rounded once; a thread per 4 columns
template <int D>
__global__ __launch_bounds__(NT) void kvattn_merge(const float *__restrict__ slabs, bf16_t *__restrict__ dkv, long n,
                                                   const KVArgs a) {
  const long e = blockIdx.x * static_cast<long>(NT) + threadIdx.x;  // (((b nhead + h) 2 + s) Tk + key) (D / 4) + c4
  if (e >= n) return;
  constexpr int Q4 = D / 4;
  const int c4 = static_cast<int>(e % Q4);
  const long r = e / Q4;
  const int key = static_cast<int>(r % a.Tk);
  const int s = static_cast<int>((r / a.Tk) & 1);
  const long bh = r / (2 * a.Tk);
  const int h = static_cast<int>(bh % a.nhead);
  const long b = bh / a.nhead;
  const size_t sz = static_cast<size_t>(2) * a.Tk * D;
  const float *src = slabs + static_cast<size_t>(bh) * a.splits * sz + (static_cast<size_t>(s) * a.Tk + key) * D + 4 * c4;
  f32x4 sum = *reinterpret_cast<const f32x4 *>(src);
  for (int p = 1; p < a.splits; ++p) {
    const f32x4 v = *reinterpret_cast<const f32x4 *>(src + p * sz);
#pragma unroll
    for (int j = 0; j < 4; ++j) sum[j] += v[j];
  }
  const float f = s ? 1.f : a.scale;
  bf16_t *dst = dkv + (static_cast<size_t>(b) * a.Tk + key) * 2 * a.C + static_cast<size_t>(s) * a.C + h * D + 4 * c4;
  *reinterpret_cast<uint2 *>(dst) = make_uint2(pack2(sum[0] * f, sum[1] * f), pack2(sum[2] * f, sum[3] * f));
}

// head width, or 0 when the kernels do not serve the shape; fills a
static int make_args(KVArgs &a, long B, long Tq, long Tk, int C, int nhead) {
  if (B < 1 || Tq < 1 || Tq > 16384 || Tk < 1 || Tk > TK || nhead < 1 || C < 1 || C % nhead) return 0;
  const int d = C / nhead;
  if (d != 32 && d != 64) return 0;
  if (Tq * C * 2 > 0x7fffffffL) return 0;  // (32-bit row offsets per sample; kv is smaller)
  a.Tq = static_cast<int>(Tq), a.Tk = static_cast<int>(Tk), a.C = C, a.nhead = nhead;
  a.nt = (a.Tq + TQ - 1) / TQ;
  a.fsplits = (a.nt + FWD_RUN - 1) / FWD_RUN;
  a.splits = (a.nt + BWD_RUN - 1) / BWD_RUN;
  a.per = (a.nt + a.splits - 1) / a.splits;
  a.splits = (a.nt + a.per - 1) / a.per;  // (equal runs may need fewer)
  if (B * nhead * (a.fsplits > a.splits ? a.fsplits : a.splits) > 0x7fffffffL) return 0;
  a.scale = d == 64 ? 0.125f : 0.17677669529663687f;
  a.sc2 = a.scale * LOG2E;
  return d;
}

}  // namespace

// Queries per tile and the backward's splits of Tq queries at head width d; -1: not served.
CXN_API int cxn_kvattn_tile(int d, long Tq, int *rows_per_tile, int *splits) {
  KVArgs a;
  if (!make_args(a, 1, Tq, 1, d, 1)) return -1;
  if (rows_per_tile) *rows_per_tile = TQ;
  if (splits) *splits = a.splits;
  return 0;
}

// fp32 workspace of cxn_kvattn_bwd: one slab [2][Tk][d] per (sample, head, split) when there is
// more than one split, else 0; -1: shape not served
CXN_API long cxn_kvattn_ws_floats(long B, long Tq, long Tk, int C, int nhead) {
  KVArgs a;
  const int d = make_args(a, B, Tq, Tk, C, nhead);
  if (!d) return -1;
  return a.splits > 1 ? B * nhead * a.splits * 2 * Tk * d : 0;
}

// out [B Tq][C] = softmax(q k^T / sqrt(d)) v per (sample, head) of q [B Tq][C] and kv [B Tk][2 C];
// lse [B nhead Tq] fp32 receives every row's log-sum-exp.  out must alias neither input.
CXN_API int cxn_kvattn_fwd(const void *q, const void *kv, void *out, float *lse, long B, long Tq, long Tk, int C,
                           int nhead, void *stream) {
  KVArgs a;
  const int d = make_args(a, B, Tq, Tk, C, nhead);
  if (!q || !kv || !out || !lse || q == out || kv == out || !d ||
      !(aligned16(q) && aligned16(kv) && aligned16(out)))
    return -1;
  const int grid = static_cast<int>(B * nhead * a.fsplits);
  const bf16_t *x = static_cast<const bf16_t *>(q), *y = static_cast<const bf16_t *>(kv);
  bf16_t *o = static_cast<bf16_t *>(out);
  if (d == 64) CXN_LAUNCH((kvattn_fwd<64>), grid, NT, 0, S_, x, y, o, lse, a);
  else CXN_LAUNCH((kvattn_fwd<32>), grid, NT, 0, S_, x, y, o, lse, a);
  RET;
}

// dq [B Tq][C] and dkv [B Tk][2 C] = the gradients of q and kv given dout [B Tq][C]; no state of
// the forward is read.  dq may be q and dkv may be kv.  slabs: fp32 workspace of ws_floats >=
// cxn_kvattn_ws_floats(..) (not touched when that is 0); -2 when it is smaller.
CXN_API int cxn_kvattn_bwd(const void *q, const void *kv, const void *dout, void *dq, void *dkv, float *slabs,
                           long ws_floats, long B, long Tq, long Tk, int C, int nhead, void *stream) {
  KVArgs a;
  const int d = make_args(a, B, Tq, Tk, C, nhead);
  if (!q || !kv || !dout || !dq || !dkv || !d || dout == dq || dout == dkv || dq == dkv ||
      !(aligned16(q) && aligned16(kv) && aligned16(dout) && aligned16(dq) && aligned16(dkv)))
    return -1;
  const long need = a.splits > 1 ? B * nhead * a.splits * 2 * Tk * d : 0;
  if (need && (!slabs || need > ws_floats || !aligned16(slabs))) return -2;
  const int grid = static_cast<int>(B * nhead * a.splits);
  const bf16_t *x = static_cast<const bf16_t *>(q), *y = static_cast<const bf16_t *>(kv);
  const bf16_t *g = static_cast<const bf16_t *>(dout);
  bf16_t *dx = static_cast<bf16_t *>(dq), *dy = static_cast<bf16_t *>(dkv);
  bf16_t *direct = need ? nullptr : dy;
  const long n = B * nhead * 2 * Tk * (d / 4);
  if (d == 64) {
    CXN_LAUNCH((kvattn_bwd<64>), grid, NT, 0, S_, x, y, g, dx, direct, slabs, a);
    if (need) CXN_LAUNCH((kvattn_merge<64>), static_cast<int>((n + NT - 1) / NT), NT, 0, S_, (const float *)slabs, dy, n, a);
  } else {
    CXN_LAUNCH((kvattn_bwd<32>), grid, NT, 0, S_, x, y, g, dx, direct, slabs, a);
    if (need) CXN_LAUNCH((kvattn_merge<32>), static_cast<int>((n + NT - 1) / NT), NT, 0, S_, (const float *)slabs, dy, n, a);
  }
  RET;
}
