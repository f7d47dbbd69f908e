// window_attention: multi-head self-attention inside ws x ws windows of an NHWC map, with a cyclic
// shift, Swin's region mask and a learned relative position bias (layers/extra.py
// WindowAttentionLayer).  The input is the fused qkv map [B H W][3 C] bf16 in attention's channel
// layout (channel s C + h d + j = component j of head h of q / k / v), d = 32; the output is
// [B H W][C].  Window (Wy, Wx) holds the tokens t = wy ws + wx at rolled-frame coordinates
// (Wy ws + wy, Wx ws + wx), which sit at map position ((y' + shift) mod H, (x' + shift) mod W);
// key j is excluded for query i when their wrap flags (y' + shift >= H, x' + shift >= W) differ.
//
//   cxn_wattn_fwd   one launch: O and the log-sum-exp of every row
//   cxn_wattn_bwd   one launch for dQ, dK, dV and per-block slabs of the bias gradient, then a
//                   fixed-order merge of the slabs onto gbias
//
// One tile, no streaming.  A (window, head) has n = ws^2 <= 64 tokens, so its Q, K, V (and dO) are
// one [64][32] bf16 tile each, 4 KiB, staged once by four 1-KiB LDS-DMAs per tile straight from the
// strided map rows: lane l of DMA w fetches 16-byte unit l & 3 of tile row 16 w + (l >> 2), whose
// byte offset is that token's map row -- the window gather and the cyclic shift are nothing but
// per-lane offsets -- and rows >= n take the out-of-range offset and arrive as zeros.  The softmax
// is a plain two-step over registers: max, exp2, sum; no running max, no rescale.
//
// Swizzle.  A tile row is 64 bytes, four 16-byte units; unit lc of row r lives at physical unit
// lc ^ swz(r), swz(r) = bit 2 of r as bit 1, bit 3 of r as bit 0.  attn_kernels.hip's r & 3 does
// not carry over to a 64-byte row: rows r and r + 4 are 256 bytes apart, all 64 banks, and would
// pick the same unit.  Model: 64 banks of 4 bytes; a 16-byte read is served 16 lanes at a time, an
// 8-byte read 32 lanes at a time.  Row-major fragment read (row_frag): 16 lanes read unit g of
// rows r0 .. r0 + 15; rows equal mod 4 share their 64 bank-bytes, and their four swz values
// are distinct, so the 16 lanes cover 16 distinct 16-byte bank groups.  Transposed read (tr_frag,
// ds_read_b64_tr_b16): 32 lanes read units 2 dt, 2 dt + 1 of rows r0 .. r0 + 7; rows r and r + 4
// differ in bit 1 of swz, which moves the unit pair {2 dt, 2 dt + 1} to the other pair.  Both are
// conflict-free under that model; bit 0 alone (rows r, r + 4 swapping inside one pair) would not be.
//
// Work split.  A block of 4 waves carries one (window, head) at a time, a wave 16 of its rows; a
// wave whose 16 rows are all past n (ws <= 6) skips the arithmetic.  Blocks are ordered head
// fastest, so the nhead blocks of one window run adjacent and together read whole qkv rows (L2
// serves the 64-byte partial-row fetches).  The forward launches one block per (window, head).  The
// backward is persistent: (sample, window) items are cut into at most PMAX / nhead runs of equal
// length, block (run, head) walks its run in order, and owns one slab of the bias gradient.
//
// Products.  As in attn_kernels.hip everything is computed transposed, S^T = K Q^T per 16 keys x
// 16 queries, so lane (i, g) holds query i and keys 4 g .. 4 g + 3 of each key tile and P^T is, as
// it stands, the B operand of O^T += V^T P^T.  The logit is mul_rn(q.k, log2e / sqrt(d)) + bias
// log2e, the bias row (2 ws - 1)^2 fp32 staged in LDS premultiplied, the relative index and the
// wrap flags of a token read from a 64-entry LDS table the staging lanes fill; the product is
// rounded on its own (mul_rn), so forward and both backward orientations form the same bits, and
// lse2 = max + log2(sum) is stored in those units: the backward's exp2(logit - lse2) is the
// forward's P.  P and dS are rounded to bf16 for the MFMAs that take them; everything else is fp32.
//
// Backward.  With the window resident D = sum_j P dP is a register sum.  Both orientations are
// recomputed rather than passed through LDS: the query orientation (D, dS, dQ = dS K) and then the
// key orientation (dK = dS^T Q, dV = P^T dO) each cost 8 MFMAs per wave for S and dP, which at
// d = 32 is less than writing and transposing two bf16 64 x 64 matrices through LDS would, and the
// LDS budget is already 16 KiB of tiles plus the 17 KiB fp32 dS below.  The row terms lse2 and D
// ride in LDS between the two.
//
// Bias gradient.  The query orientation writes its unrounded fp32 dS to an LDS matrix [key][query]
// (row stride 68 floats: the four key rows of a store land 16 banks apart).  Thread r < (2 ws - 1)^2
// then sums, over the keys in token order, the one query at relative index r of each key, adds the
// window's sum to its register total in window order, and stores the total to the block's slab at
// the end.  wattn_merge adds the slabs in run order onto gbias (ln_kernels.hip's merge).  No
// atomics anywhere: the same bits on every run.
//
// Aliasing.  dqkv may be qkv.  A block's DMAs have fetched every q, k and v row of its (window,
// head) -- the block barrier after vmcnt(0) -- before any of its waves stores, it reads only LDS
// after that, and no other block ever reads those columns of those rows.  So the gradient goes in
// place with no staging buffer and no extra launch.  Keep that order: stage, barrier, then stores.
//
// Hazards.  P and dS are VALU results feeding MFMA operands: every MFMA is the compiler builtin
// (see attn_kernels.hip).  The DMAs are the asm form; completion is vmcnt(0) plus a block barrier.
#include "attn_tile.h"

using namespace cxg;
using namespace cxg::attn::row64;  // swz, tile_addr, row_frag, tr_frag of the [64][32] tile

namespace {

constexpr int NT = 256;
constexpr int TR = 64;            // rows of a tile
constexpr int D = 32;             // head width
constexpr int TILE = TR * D * 2;  // bytes
constexpr int DSS = 68;           // row stride of the fp32 dS matrix, floats
constexpr int RMAX = 225;         // (2 ws - 1)^2 at ws = 8
constexpr int PMAX = 768;         // backward: blocks (bias-gradient slabs) at most
constexpr uint32_t OOB = 0x80000000u;  // >= num_records: the DMA writes zeros
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
// token table entry: bits 0..7 wy (2 ws - 1) + wx, bit 8 / 9 the y / x wrap flag, bit 10 "exists"
constexpr uint32_t M_REL = 0xffu, M_WRAP = 0x300u, M_OK = 0x400u;

struct WArgs {
  int H, W, C, nhead, ws, shift, n;  // map, channels of one of q / k / v, heads, window, tokens of a window
  int nwx, nwin, R, ctr;             // windows per map row / per sample, bias row length, index of (0, 0)
  long items, per;                   // (sample, window) items; backward: items per run
  float sc2, scale;                  // log2e / sqrt(d), 1 / sqrt(d)
};

__device__ __forceinline__ f32x4 mma(const bf16x8 &a, const bf16x8 &b, const f32x4 &c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// a b rounded to fp32 on its own: the empty asm keeps hipcc from contracting it into the bias add
__device__ __forceinline__ float mul_rn(float a, float b) {
  float x = a * b;
  asm("" : "+v"(x));
  return x;
}

__device__ __forceinline__ bf16x8 pack_frag(const f32x4 &lo, const f32x4 &hi) {
  const uint4 v = make_uint4(pack2(lo[0], lo[1]), pack2(lo[2], lo[3]), pack2(hi[0], hi[1]), pack2(hi[2], hi[3]));
  return __builtin_bit_cast(bf16x8, v);
}

// 4 columns 16 dt + 4 g .. of a row for both dt, scaled
__device__ __forceinline__ void store_row(bf16_t *row, int g, const f32x4 (&acc)[2], float f) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
    *reinterpret_cast<uint2 *>(row + 16 * dt + 4 * g) =
        make_uint2(pack2(acc[dt][0] * f, acc[dt][1] * f), pack2(acc[dt][2] * f, acc[dt][3] * f));
}

__device__ __forceinline__ uint32_t lds_base(const char *smem) {
  return __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_void *)smem)));
}

struct Item {
  int b, Wy, Wx;
};
__device__ __forceinline__ Item item_of(long it, const WArgs &a) {
  Item w;
  w.b = static_cast<int>(it / a.nwin);
  const int win = static_cast<int>(it - static_cast<long>(w.b) * a.nwin);
  w.Wy = win / a.nwx;
  w.Wx = win - w.Wy * a.nwx;
  return w;
}

// token t of window (Wy, Wx): its map row y W + x (-1 past the window) and its table entry
__device__ __forceinline__ void tok_info(int t, const Item &w, const WArgs &a, int &row, uint32_t &meta) {
  const int wy = t / a.ws, wx = t - wy * a.ws;
  const int yr = w.Wy * a.ws + wy + a.shift, xr = w.Wx * a.ws + wx + a.shift;
  const bool fy = yr >= a.H, fx = xr >= a.W, ok = t < a.n;
  row = ok ? (fy ? yr - a.H : yr) * a.W + (fx ? xr - a.W : xr) : -1;
  meta = ok ? static_cast<uint32_t>(wy * (2 * a.ws - 1) + wx) | (fy ? 0x100u : 0u) | (fx ? 0x200u : 0u) | M_OK : 0u;
}

// key tk for a query with table entry mq (okq: the query exists): is it attended, and the bias index
__device__ __forceinline__ bool pair(uint32_t mq, bool okq, uint32_t mk, int ctr, int &idx) {
  const bool on = okq && (mk & M_OK) && (mk & M_WRAP) == (mq & M_WRAP);
  idx = on ? static_cast<int>(mq & M_REL) - static_cast<int>(mk & M_REL) + ctr : 0;
  return on;
}

// ------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(NT) void wattn_fwd(const bf16_t *__restrict__ qkv, bf16_t *__restrict__ out,
                                                const float *__restrict__ bias, float *__restrict__ lse,
                                                float *__restrict__ lse2, const WArgs a) {
  __shared__ __attribute__((aligned(1024))) char smem[3 * TILE];  // Q | K | V
  __shared__ float s_bias[RMAX + 7];
  __shared__ int s_row[TR];
  __shared__ uint32_t s_meta[TR];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int h = blockIdx.x % a.nhead;
  const Item w = item_of(blockIdx.x / a.nhead, a);
  const size_t HW = static_cast<size_t>(a.H) * a.W, rs = 3 * static_cast<size_t>(a.C);
  const bf16_t *base = qkv + static_cast<size_t>(w.b) * HW * rs + h * D;
  const uint32_t rsb = static_cast<uint32_t>(rs) * 2u, nrec = static_cast<uint32_t>(HW - 1) * rsb + D * 2u;
  const uint32_t lds0 = lds_base(smem);

  {  // stage: DMA `wave` of each tile is rows 16 wave .. 16 wave + 15
    const int r = wave * 16 + (lane >> 2), pc = lane & 3;
    int row;
    uint32_t meta;
    tok_info(r, w, a, row, meta);
    uint32_t off = row >= 0 ? static_cast<uint32_t>(row) * rsb + static_cast<uint32_t>(pc ^ swz(r)) * 16u : OOB;
    asm volatile("" : "+v"(off));  // keep the select: no per-lane branch around the DMA
#pragma unroll
    for (int s = 0; s < 3; ++s) dma16(make_rsrc(base + s * a.C, nrec), lds0 + s * TILE + wave * 1024, off);
    if (pc == 0) {
      s_row[r] = row;
      s_meta[r] = meta;
    }
    if (tid < a.R) s_bias[tid] = bias[h * a.R + tid] * LOG2E;
  }
  wait_vmcnt<0>();
  __syncthreads();
  if (wave * 16 >= a.n) return;  // (no barrier follows)

  const char *qb = smem, *kb = smem + TILE, *vb = smem + 2 * TILE;
  const int tq = wave * 16 + i;
  const uint32_t mq = s_meta[tq];
  const bool okq = mq & M_OK;
  const bf16x8 qf = row_frag(qb, tq, g);
  f32x4 s[4];
  float m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    s[kt] = mma(row_frag(kb, 16 * kt + i, g), qf, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int idx;
      const bool on = pair(mq, okq, s_meta[16 * kt + 4 * g + j], a.ctr, idx);
      const float v = mul_rn(s[kt][j], a.sc2) + s_bias[idx];
      s[kt][j] = on ? v : -INFINITY;
      m = fmaxf(m, s[kt][j]);
    }
  }
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  if (!okq) m = 0.f;  // a row past the window: every P below is exp2(-inf) = 0
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
  f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int kp = 0; kp < 2; ++kp) {
    const bf16x8 pf = pack_frag(s[2 * kp], s[2 * kp + 1]);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) o[dt] = mma(tr_frag(vb, 32 * kp, dt, i, g), pf, o[dt]);
  }
  if (okq) {
    const size_t row = static_cast<size_t>(s_row[tq]);
    store_row(out + (static_cast<size_t>(w.b) * HW + row) * a.C + h * D, g, o, 1.f / l);
    if (g == 0) {
      const float v = m + log2f(l);
      const size_t e = (static_cast<size_t>(w.b) * a.nhead + h) * HW + row;
      lse[e] = v * LN2;
      lse2[e] = v;
    }
  }
}

// ------------------------------------------------------------------------------------ backward
// Block (run, head) = blockIdx.x walks items run per .. of head h.  dqkv null: the bias gradient only.
__global__ __launch_bounds__(NT) void wattn_bwd(const bf16_t *qkv, const bf16_t *__restrict__ dout,
                                                const float *__restrict__ bias, const float *__restrict__ lse2,
                                                bf16_t *dqkv, float *__restrict__ slabs, const WArgs a) {
  __shared__ __attribute__((aligned(1024))) char smem[4 * TILE];  // Q | K | V | dO
  __shared__ float s_ds[TR * DSS];                                // fp32 dS [key][query]
  __shared__ float s_bias[RMAX + 7], s_stat[2][TR];               // [lse2 | D][query]
  __shared__ int s_row[TR];
  __shared__ uint32_t s_meta[TR];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int h = blockIdx.x % a.nhead;
  const long run = blockIdx.x / a.nhead;
  const size_t HW = static_cast<size_t>(a.H) * a.W, rs = 3 * static_cast<size_t>(a.C);
  const uint32_t rsb = static_cast<uint32_t>(rs) * 2u, gsb = static_cast<uint32_t>(a.C) * 2u;
  const uint32_t nrec = static_cast<uint32_t>(HW - 1) * rsb + D * 2u, grec = static_cast<uint32_t>(HW - 1) * gsb + D * 2u;
  const uint32_t lds0 = lds_base(smem);
  const char *qb = smem, *kb = smem + TILE, *vb = smem + 2 * TILE, *gb = smem + 3 * TILE;

  // the relative offset this thread sums: tid = (dy + ws - 1) (2 ws - 1) + dx + ws - 1
  const int ry = tid / (2 * a.ws - 1) - (a.ws - 1), rx = tid % (2 * a.ws - 1) - (a.ws - 1);
  float gsum = 0.f;
  if (tid < a.R) s_bias[tid] = bias[h * a.R + tid] * LOG2E;

  const long it1 = (run + 1) * a.per < a.items ? (run + 1) * a.per : a.items;
  for (long it = run * a.per; it < it1; ++it) {
    const Item w = item_of(it, a);
    const bf16_t *base = qkv + static_cast<size_t>(w.b) * HW * rs + h * D;
    const float *l2p = lse2 + (static_cast<size_t>(w.b) * a.nhead + h) * HW;
    {
      const int r = wave * 16 + (lane >> 2), pc = lane & 3;
      int row;
      uint32_t meta;
      tok_info(r, w, a, row, meta);
      const uint32_t lc16 = static_cast<uint32_t>(pc ^ swz(r)) * 16u;
      uint32_t off = row >= 0 ? static_cast<uint32_t>(row) * rsb + lc16 : OOB;
      uint32_t goff = row >= 0 ? static_cast<uint32_t>(row) * gsb + lc16 : OOB;
      asm volatile("" : "+v"(off), "+v"(goff));
#pragma unroll
      for (int s = 0; s < 3; ++s) dma16(make_rsrc(base + s * a.C, nrec), lds0 + s * TILE + wave * 1024, off);
      dma16(make_rsrc(dout + static_cast<size_t>(w.b) * HW * a.C + h * D, grec), lds0 + 3 * TILE + wave * 1024, goff);
      if (pc == 0) {
        s_row[r] = row;
        s_meta[r] = meta;
        s_stat[0][r] = row >= 0 ? l2p[row] : 0.f;
      }
    }
    wait_vmcnt<0>();
    __syncthreads();  // the whole (window, head) is in LDS: stores may follow (in-place gradient)

    const bool busy = wave * 16 < a.n;
    if (busy) {  // query orientation: the wave's 16 queries against all keys
      const int tq = wave * 16 + i;
      const uint32_t mq = s_meta[tq];
      const bool okq = mq & M_OK;
      const bf16x8 qf = row_frag(qb, tq, g), gf = row_frag(gb, tq, g);
      const float l2 = s_stat[0][tq];
      f32x4 p[4], dp[4];
      float dsl = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        p[kt] = mma(row_frag(kb, 16 * kt + i, g), qf, f32x4{0.f, 0.f, 0.f, 0.f});
        dp[kt] = mma(row_frag(vb, 16 * kt + i, g), gf, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          int idx;
          const bool on = pair(mq, okq, s_meta[16 * kt + 4 * g + j], a.ctr, idx);
          const float v = mul_rn(p[kt][j], a.sc2) + s_bias[idx];
          p[kt][j] = on ? __builtin_amdgcn_exp2f(v - l2) : 0.f;
          dsl = fmaf(p[kt][j], dp[kt][j], dsl);
        }
      }
      dsl += __shfl_xor(dsl, 16, 64);
      dsl += __shfl_xor(dsl, 32, 64);
      if (g == 0) s_stat[1][tq] = dsl;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          p[kt][j] *= dp[kt][j] - dsl;  // dS
          s_ds[(16 * kt + 4 * g + j) * DSS + tq] = p[kt][j];
        }
      if (dqkv) {
        f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int kp = 0; kp < 2; ++kp) {
          const bf16x8 df = pack_frag(p[2 * kp], p[2 * kp + 1]);
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) acc[dt] = mma(tr_frag(kb, 32 * kp, dt, i, g), df, acc[dt]);
        }
        if (okq)
          store_row(dqkv + (static_cast<size_t>(w.b) * HW + static_cast<size_t>(s_row[tq])) * rs + h * D, g, acc, a.scale);
      }
    }
    __syncthreads();  // D and the fp32 dS are in LDS

    if (busy && dqkv) {  // key orientation: the wave's 16 keys against all queries
      const int tk = wave * 16 + i;
      const uint32_t mk = s_meta[tk];
      const bool okk = mk & M_OK;
      const bf16x8 kf = row_frag(kb, tk, g), vf = row_frag(vb, tk, g);
      f32x4 p[4], ds[4];
#pragma unroll
      for (int qt = 0; qt < 4; ++qt) {
        p[qt] = mma(row_frag(qb, 16 * qt + i, g), kf, f32x4{0.f, 0.f, 0.f, 0.f});
        ds[qt] = mma(row_frag(gb, 16 * qt + i, g), vf, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int tq = 16 * qt + 4 * g + j;
          const uint32_t mq = s_meta[tq];
          int idx;
          const bool on = pair(mq, mq & M_OK, okk ? mk : 0u, a.ctr, idx);
          const float v = mul_rn(p[qt][j], a.sc2) + s_bias[idx];
          p[qt][j] = on ? __builtin_amdgcn_exp2f(v - s_stat[0][tq]) : 0.f;
          ds[qt][j] = on ? p[qt][j] * (ds[qt][j] - s_stat[1][tq]) : 0.f;  // (D of an idle wave's rows is unwritten)
        }
      }
      f32x4 dk[2], dv[2];
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) dk[dt] = dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int qp = 0; qp < 2; ++qp) {
        const bf16x8 pf = pack_frag(p[2 * qp], p[2 * qp + 1]), df = pack_frag(ds[2 * qp], ds[2 * qp + 1]);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dv[dt] = mma(tr_frag(gb, 32 * qp, dt, i, g), pf, dv[dt]);
          dk[dt] = mma(tr_frag(qb, 32 * qp, dt, i, g), df, dk[dt]);
        }
      }
      if (okk) {
        bf16_t *orow = dqkv + (static_cast<size_t>(w.b) * HW + static_cast<size_t>(s_row[tk])) * rs + h * D;
        store_row(orow + a.C, g, dk, a.scale);
        store_row(orow + 2 * a.C, g, dv, 1.f);
      }
    }
    if (tid < a.R) {  // sum over the keys, in token order, of dS[query = key + (ry, rx)][key]
      float sum = 0.f;
      int ky = 0, kx = 0;
      for (int tk = 0; tk < a.n; ++tk) {
        const int qy = ky + ry, qx = kx + rx;
        const bool in = qy >= 0 && qy < a.ws && qx >= 0 && qx < a.ws;
        const float v = s_ds[tk * DSS + (in ? qy * a.ws + qx : 0)];
        sum += in ? v : 0.f;
        if (++kx == a.ws) {
          kx = 0;
          ++ky;
        }
      }
      gsum += sum;
    }
    __syncthreads();  // every reader of the tiles and tables is done: the next item may land
  }
  if (tid < a.R) slabs[static_cast<size_t>(blockIdx.x) * a.R + tid] = gsum;
}

// gbias[h][r] += sum over the runs of slab (run, h)[r], in run order
__global__ __launch_bounds__(NT) void wattn_merge(const float *__restrict__ slabs, int runs, int n, float *gbias) {
  const int e = blockIdx.x * NT + threadIdx.x;  // h R + r
  if (e >= n) return;
  float sum = 0.f;
  for (int p = 0; p < runs; ++p) sum += slabs[static_cast<size_t>(p) * n + e];
  gbias[e] += sum;
}

// false: the kernels do not serve the shape
static bool make_args(WArgs &a, long B, int H, int W, int C, int nhead, int ws, int shift) {
  if (B < 1 || H < 1 || W < 1 || nhead < 1 || C != nhead * D) return false;
  if (ws < 1 || ws * ws > TR || H % ws || W % ws || shift < 0 || shift >= ws) return false;
  if (static_cast<long>(H) * W * 3 * C * 2 > 0x7fffffffL) return false;  // (32-bit row offsets per sample)
  a.H = H, a.W = W, a.C = C, a.nhead = nhead, a.ws = ws, a.shift = shift, a.n = ws * ws;
  a.nwx = W / ws;
  a.nwin = (H / ws) * a.nwx;
  a.R = (2 * ws - 1) * (2 * ws - 1);
  a.ctr = (ws - 1) * (2 * ws - 1) + ws - 1;
  a.items = B * a.nwin;
  if (a.items * nhead > 0x7fffffffL) return false;
  // the backward's cut: at most PMAX / nhead runs of equal length, a function of the shape alone
  const long cap = PMAX / nhead > 1 ? PMAX / nhead : 1;
  a.per = (a.items + cap - 1) / cap;
  a.scale = 0.17677669529663687f;
  a.sc2 = a.scale * LOG2E;
  return true;
}

static long runs_of(const WArgs &a) { return (a.items + a.per - 1) / a.per; }

}  // namespace

// fp32 workspace of cxn_wattn_bwd: one slab of (2 ws - 1)^2 floats per (run, head); 0: shape not served
CXN_API long cxn_wattn_ws_floats(long B, int H, int W, int C, int nhead, int ws, int shift) {
  WArgs a;
  if (!make_args(a, B, H, W, C, nhead, ws, shift)) return 0;
  return runs_of(a) * nhead * a.R;
}

// out [B H W][C] = windowed softmax(q k^T / sqrt(d) + bias, masked) v of qkv [B H W][3 C]; bias
// [nhead][(2 ws - 1)^2] fp32; lse and lse2 [B nhead H W] fp32 receive every row's log-sum-exp in
// natural and in the kernel's log2 units, at the row's map position.  out must not alias qkv.
CXN_API int cxn_wattn_fwd(const void *qkv, void *out, const float *bias, float *lse, float *lse2, long B, int H,
                          int W, int C, int nhead, int ws, int shift, void *stream) {
  WArgs a;
  if (!qkv || !out || !bias || !lse || !lse2 || qkv == out || !make_args(a, B, H, W, C, nhead, ws, shift) ||
      !(aligned16(qkv) && aligned16(out)))
    return -1;
  const int grid = static_cast<int>(a.items * nhead);
  CXN_LAUNCH((wattn_fwd), grid, NT, 0, S_, static_cast<const bf16_t *>(qkv), static_cast<bf16_t *>(out), bias, lse,
             lse2, a);
  RET;
}

// gbias [nhead][(2 ws - 1)^2] += the bias gradient; dqkv (nullable: parameter gradient only; may be
// qkv) = the gradient of qkv given dout [B H W][C] and the forward's lse2.  slabs: fp32 workspace of
// ws_floats >= cxn_wattn_ws_floats(..); -2 when it is smaller.
CXN_API int cxn_wattn_bwd(const void *qkv, const void *dout, const float *bias, const float *lse2, void *dqkv,
                          float *gbias, float *slabs, long ws_floats, long B, int H, int W, int C, int nhead, int ws,
                          int shift, void *stream) {
  WArgs a;
  if (!qkv || !dout || !bias || !lse2 || !gbias || dout == dqkv || !make_args(a, B, H, W, C, nhead, ws, shift) ||
      !(aligned16(qkv) && aligned16(dout) && aligned16(dqkv)))
    return -1;
  const int runs = static_cast<int>(runs_of(a)), n = nhead * a.R;
  if (!slabs || static_cast<long>(runs) * n > ws_floats) return -2;
  CXN_LAUNCH((wattn_bwd), runs * nhead, NT, 0, S_, static_cast<const bf16_t *>(qkv),
             static_cast<const bf16_t *>(dout), bias, lse2, static_cast<bf16_t *>(dqkv), slabs, a);
  CXN_LAUNCH((wattn_merge), (n + NT - 1) / NT, NT, 0, S_, (const float *)slabs, runs, n, gbias);
  RET;
}
