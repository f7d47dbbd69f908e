// neighborhood_attention: every pixel of an NHWC map attends the k x k pixels around it, NAT's
// clamped neighbourhood, with a learned relative position bias (layers/extra.py
// NeighborhoodAttentionLayer).  The input is the fused qkv map [B H W][3 C] bf16 in attention's
// channel layout (channel s C + h d + j = component j of head h of q / k / v), d = 32, k = 3, 5, 7;
// the output is [B H W][C].  The query at (y, x) has the keys (y', x') with sy <= y' < sy + k,
// sx <= x' < sx + k, sy = clamp(y - k / 2, 0, H - k), sx likewise: always k^2 keys, nothing padded.
//
//   cxn_nattn_fwd   one launch: O and the log-sum-exp of every row
//   cxn_nattn_bwd   query orientation (D, dQ, bias-gradient slabs), a fixed-order merge of the
//                   slabs onto gbias, key orientation (dK, dV), and -- in place only -- a copy of dQ
//
// Patch and halo.  A block of 4 waves carries an 8 x 8 patch of one (sample, head); a wave takes two
// patch rows, 16 pixels: lane (i, g) has pixel (2 wave + (i >> 3), i & 7).  sy is monotone and
// 1-Lipschitz in y, so the neighbourhoods of a patch lie in the HS x HS square, HS = 8 + k - 1, at
// (sy(y0), sx(x0)): the key halo.  K and V of the halo are staged once by LDS-DMA as [NR][32] bf16
// tiles, row hy HS + hx: lane l of DMA w fetches 16-byte unit l & 3 of tile row 16 w + (l >> 2)
// straight from the strided qkv row of that pixel, and a row past the square or the map takes the
// out-of-range offset and arrives as zeros (so a masked key's V is a finite number, and 0 P V = 0).
// At k = 7 that is 196 keys in 224 rows, 28 KiB for K and V.  The pixels' own rows (q, dO; k, v in
// the key orientation) are 16 bytes per lane straight from memory.  wattn_kernels.hip's 64-byte-row
// swizzle is kept (attn_tile.h, row64); its argument needs 16 (8) consecutive rows, not an aligned start, so a fragment
// may begin at any tile row.
//
// Work per wave.  The two rows of a wave see k + 1 halo rows, (k + 1) HS consecutive tile rows
// from (sy(first row) - sy(y0)) HS: 112 keys, seven 16-key tiles at k = 7 (5 at k = 5, 3 at k = 3),
// and it multiplies those and no others: 49 of 112 products are attended, 44 % (all 196: 25 %).
//
// Products.  As in attn_kernels.hip everything is computed transposed, S^T = K Q^T per 16 keys x
// 16 queries, so lane (i, g) holds query i and keys 4 g .. 4 g + 3 of each tile and P^T is, as it
// stands, the B operand of O^T += V^T P^T (an odd last tile pairs with zeros).  The halo coordinates
// of a key are a division of its tile row by the constant HS; membership is the definition's own
// test on them, and a key outside gets -inf, probability exactly 0.  The softmax is a plain two-step
// over registers -- the whole neighbourhood is resident: max, exp2, sum.  The logit is
// mul_rn(q.k, log2e / sqrt(d)) + bias log2e, the bias row (2 k - 1)^2 fp32 in LDS premultiplied;
// the product is rounded on its own, so the forward and both backward orientations form the same
// bits and the backward's exp2(logit - lse2) is the forward's P (lse2 = max + log2(sum) is stored in
// those units; the backward does not normalise again).  P and dS are rounded to bf16 for the MFMAs
// that take them; everything else is fp32.
//
// Backward, query orientation (nattn_bwd_q): the forward's geometry with V and dO beside K and Q.
// D = sum_j P dP is a register sum and is also stored for the key orientation; dQ = dS K.  The
// kernel is persistent, (sample, patch) items cut into at most PMAX / nhead runs of equal length, a
// function of the shape alone; block (run, head) owns one slab of the bias gradient.
//
// Backward, key orientation (nattn_bwd_kv): a block is the same 8 x 8 patch, now of keys, a lane one
// key with k and v in registers.  Under clamping the queries that attend key row y' are NOT the
// mirror image: rows lo(y') .. hi(y'), lo = 0 for y' <= k - 1 else y' - k / 2, hi = H - 1 for
// y' >= H - k else y' + k / 2 -- up to k - 1 away on a border side -- so a patch's query halo is up
// to QS = 8 + (k - 1) + k / 2 rows and columns (k = 7, H = 22: key rows 8 .. 15 have query rows
// 5 .. 21).  Q and dO of that square are staged like the key halo (289 rows in 320, 40 KiB), lse2,
// D and the coordinates of every staged query sit in LDS tables, and a wave walks, 32 queries at a
// time, only the halo rows lo(first) .. hi(second) of its two key rows: 2 + (k - 1) + k / 2 rows at
// most in a map of more than 2 k rows (all of a smaller one), 12 tiles at k = 7, of which 49 of 192
// products are attended, 25 %; a wave in the interior has 2 + (k - 1) rows, 8 tiles, 38 %.
// Membership is decided by the forward's test from the query's side, sy(y) <= y' < sy(y) + k, never
// by a distance.  Nothing waits on the whole row here, so P and dS are consumed pair by pair and
// dK, dV are 16 accumulator registers.  No sum crosses a wave or a block.
//
// Bias gradient.  The query orientation writes its unrounded fp32 dS to LDS in lane order (one
// 16-byte store per lane and tile, conflict-free).  Thread r < (2 k - 1)^2 then adds, over the 64
// queries of the patch in order, the one key at relative offset r of each query, adds the patch's
// sum to its register total in item order and stores the total to the block's slab at the end;
// nattn_merge adds the slabs in run order onto gbias.  No atomics anywhere: the same bits every run.
//
// Aliasing.  dqkv may be qkv, but unlike the window kernels another block's halo reads the rows a
// block's gradient would overwrite.  The order of the launches settles it: the query orientation
// reads k and v of other blocks and writes only dQ; the key orientation reads q of other blocks and
// writes only dK and dV of its own pixels, each wave after its own loads of them.  So the one
// conflict is dQ over q before the key orientation has read q: in place, dQ goes to a [B H W][C]
// staging buffer and a copy launch after the key orientation moves it; out of place it is written
// directly.  An in-place call without the staging buffer is refused.
//
// Hazards.  P and dS are VALU results feeding MFMA operands: every MFMA is the compiler builtin
// (see attn_kernels.hip).  The DMAs are the asm form; completion is vmcnt(0) plus a block barrier.
#include "attn_tile.h"

using namespace cxg;
using namespace cxg::attn;
using namespace cxg::attn::row64;  // swz, tile_addr, row_frag, tr_frag of the [rows][32] tile

namespace {

constexpr int NT = 256;
constexpr int D = 32;      // head width
constexpr int PS = 8;      // patch side
constexpr int PMAX = 768;  // backward: blocks of the query orientation (bias-gradient slabs) at most

template <int K>
struct Geo {
  static constexpr int HS = PS + K - 1;                                      // key halo side
  static constexpr int NKT = ((K + 1) * HS + 15) / 16;                       // key tiles of a wave
  // rows of a key halo tile: a wave starts at most 6 halo rows down and reads whole tile pairs
  static constexpr int NR = (6 * HS + 32 * ((NKT + 1) / 2) + 15) / 16 * 16;
  static constexpr int QS = PS + K - 1 + K / 2;                              // query halo side
  // rows of a query halo tile: a wave's last 32-query step may overhang the square
  static constexpr int NRQ = (QS * QS + 31 + 15) / 16 * 16;
  static constexpr int R = (2 * K - 1) * (2 * K - 1);                        // bias row
  static_assert(NR >= HS * HS && NRQ >= QS * QS, "the halo must fit its tile");
};

struct NArgs {
  int H, W, C, nhead;  // map, channels of one of q / k / v, heads
  int npx, npatch;     // patches per map row / per sample
  long items, per;     // (sample, patch) items; query orientation: items per run
  float sc2, scale;    // log2e / sqrt(d), 1 / sqrt(d)
};

// clamp(v, 0, hi): the start of a neighbourhood is nb<K>(y, H) = clamp(y - K / 2, 0, H - K)
__device__ __forceinline__ int clamp0(int v, int hi) { return min(max(v, 0), hi); }
template <int K>
__device__ __forceinline__ int nb(int y, int H) { return clamp0(y - K / 2, H - K); }
// first and last query row (column) that attends key row (column) y of a map of H rows (columns)
template <int K>
__device__ __forceinline__ int lo_q(int y) { return y <= K - 1 ? 0 : y - K / 2; }
template <int K>
__device__ __forceinline__ int hi_q(int y, int H) { return y >= H - K ? H - 1 : y + K / 2; }

struct Patch {
  int b, y0, x0;
};
__device__ __forceinline__ Patch patch_of(long it, const NArgs &a) {
  Patch p;
  p.b = static_cast<int>(it / a.npatch);
  const int pp = static_cast<int>(it - static_cast<long>(p.b) * a.npatch);
  const int py = pp / a.npx;
  p.y0 = py * PS;
  p.x0 = (pp - py * a.npx) * PS;
  return p;
}

// Stage the SIDE x SIDE square of pixels at (oy, ox) of two strided matrices (descriptors ra / rb,
// row strides sa / sb bytes, 32 columns each) into the [ROWS][32] tiles at lds and lds + ROWS 64,
// tile row hy SIDE + hx.  Wave w issues DMAs w, w + 4, ..; rows past the square or the map get zeros.
template <int SIDE, int ROWS>
__device__ __forceinline__ void stage_halo(rsrc_t ra, uint32_t sa, rsrc_t rb, uint32_t sb, uint32_t lds, int oy, int ox,
                                           int H, int W, int wave, int lane) {
#pragma unroll
  for (int q0 = 0; q0 < ROWS / 16; q0 += 4) {
    const int q = q0 + wave;
    if (q < ROWS / 16) {
      const int r = q * 16 + (lane >> 2), hy = r / SIDE, hx = r - hy * SIDE;
      const bool ok = hy < SIDE && oy + hy < H && ox + hx < W;
      const uint32_t pix = static_cast<uint32_t>((oy + hy) * W + ox + hx);
      const uint32_t u = static_cast<uint32_t>((lane & 3) ^ swz(r)) * 16u;
      uint32_t offa = ok ? pix * sa + u : OOB, offb = ok ? pix * sb + u : OOB;
      asm volatile("" : "+v"(offa), "+v"(offb));  // keep the selects: no per-lane branch around the DMAs
      dma16(ra, lds + static_cast<uint32_t>(q * 1024), offa);
      dma16(rb, lds + static_cast<uint32_t>(ROWS * D * 2 + q * 1024), offb);
    }
  }
}

// what a lane of the query orientation knows of its query: the pixel, whether it exists, and the
// constants of the membership test and the bias index in halo coordinates
template <int K>
struct Query {
  int y, x, ly, lx, cq, kb0;
  bool ok;
  // wave's rows y0 + 2 wave, + 1; halo origin (hy0, hx0)
  __device__ __forceinline__ Query(const Patch &p, int hy0, int hx0, int wave, int i, const NArgs &a) {
    const int yw = p.y0 + 2 * wave;
    y = yw + (i >> 3), x = p.x0 + (i & 7);
    ok = y < a.H && x < a.W;
    ly = ok ? nb<K>(y, a.H) - hy0 : 1 << 20;  // (no halo row passes the test of a pixel off the map)
    lx = nb<K>(x, a.W) - hx0;
    cq = (hy0 - y + K - 1) * (2 * K - 1) + hx0 - x + K - 1;
    kb0 = (nb<K>(yw, a.H) - hy0) * Geo<K>::HS;
  }
  // tile row n of the key halo: attended?  idx: its bias index (0 when not)
  __device__ __forceinline__ bool pair(int n, int &idx) const {
    const int hy = n / Geo<K>::HS, hx = n - hy * Geo<K>::HS;
    const bool on = static_cast<unsigned>(hy - ly) < static_cast<unsigned>(K) &&
                    static_cast<unsigned>(hx - lx) < static_cast<unsigned>(K);
    idx = on ? hy * (2 * K - 1) + hx + cq : 0;
    return on;
  }
};

__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// ------------------------------------------------------------------------------------ forward
template <int K>
__global__ __launch_bounds__(NT) void nattn_fwd(const bf16_t *__restrict__ qkv, bf16_t *__restrict__ out,
                                                const float *__restrict__ bias, float *__restrict__ lse,
                                                float *__restrict__ lse2, const NArgs a) {
  using G = Geo<K>;
  constexpr int NKT = G::NKT, TILE = G::NR * D * 2;
  __shared__ __attribute__((aligned(1024))) char smem[2 * TILE];  // K | V
  __shared__ float s_bias[G::R + 7];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int h = blockIdx.x % a.nhead;
  const Patch p = patch_of(blockIdx.x / a.nhead, a);
  const int hy0 = nb<K>(p.y0, a.H), hx0 = nb<K>(p.x0, a.W);
  const size_t HW = static_cast<size_t>(a.H) * a.W, rs = 3 * static_cast<size_t>(a.C);
  const bf16_t *base = qkv + static_cast<size_t>(p.b) * HW * rs + h * D;
  const uint32_t rsb = static_cast<uint32_t>(rs) * 2u, nrec = static_cast<uint32_t>(HW - 1) * rsb + D * 2u;

  stage_halo<G::HS, G::NR>(make_rsrc(base + a.C, nrec), rsb, make_rsrc(base + 2 * a.C, nrec), rsb, lds_base(smem), hy0,
                           hx0, a.H, a.W, wave, lane);
  if (tid < G::R) s_bias[tid] = bias[h * G::R + tid] * LOG2E;
  const Query<K> q(p, hy0, hx0, wave, i, a);
  const size_t pix = static_cast<size_t>(q.y) * a.W + q.x;
  bf16x8 qf[1];
  load_row<1>(base + pix * rs, q.ok, g, qf);
  wait_vmcnt<0>();
  __syncthreads();
  if (p.y0 + 2 * wave >= a.H) return;  // (no barrier follows)

  const char *kb = smem, *vb = smem + TILE;
  const int n0 = q.kb0 + 4 * g;
  f32x4 s[NKT];
  float m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    s[kt] = mma(row_frag(kb, q.kb0 + 16 * kt + i, g), qf[0], zero4());
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int idx;
      const bool on = q.pair(n0 + 16 * kt + j, idx);
      const float v = mul_rn(s[kt][j], a.sc2) + s_bias[idx];
      s[kt][j] = on ? v : -INFINITY;
      m = fmaxf(m, s[kt][j]);
    }
  }
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  if (!q.ok) m = 0.f;  // a pixel off the map: every P below is exp2(-inf) = 0
  float l = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[kt][j] = __builtin_amdgcn_exp2f(s[kt][j] - m);
      l += s[kt][j];
    }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  f32x4 o[2] = {zero4(), zero4()};
#pragma unroll
  for (int kp = 0; kp < (NKT + 1) / 2; ++kp) {
    const bf16x8 pf = pack_frag(s[2 * kp], 2 * kp + 1 < NKT ? s[2 * kp + 1 < NKT ? 2 * kp + 1 : 0] : zero4());
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) o[dt] = mma(tr_frag(vb, q.kb0 + 32 * kp, dt, i, g), pf, o[dt]);
  }
  if (q.ok) {
    store_row<2>(out + (static_cast<size_t>(p.b) * HW + pix) * a.C + h * D, g, o, 1.f / l);
    if (g == 0) {
      const float v = m + log2f(l);
      const size_t e = (static_cast<size_t>(p.b) * a.nhead + h) * HW + pix;
      lse[e] = v * LN2;
      lse2[e] = v;
    }
  }
}

// --------------------------------------------------------------- backward, query orientation
// Block (run, head) = blockIdx.x walks items run per .. of head h: D of every query into dsum, the
// bias gradient into the block's slab, and dQ (dq null: not wanted) into rows of dqs elements.
template <int K>
__global__ __launch_bounds__(NT) void nattn_bwd_q(const bf16_t *__restrict__ qkv, const bf16_t *__restrict__ dout,
                                                  const float *__restrict__ bias, const float *__restrict__ lse2,
                                                  float *__restrict__ dsum, bf16_t *__restrict__ dq, long dqs,
                                                  float *__restrict__ slabs, const NArgs a) {
  using G = Geo<K>;
  constexpr int NKT = G::NKT, HS = G::HS, TILE = G::NR * D * 2;
  __shared__ __attribute__((aligned(1024))) char smem[2 * TILE];  // K | V
  __shared__ f32x4 s_ds[4 * NKT * 64];                            // fp32 dS [wave][tile][lane]
  __shared__ float s_bias[G::R + 7];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int h = blockIdx.x % a.nhead;
  const long run = blockIdx.x / a.nhead;
  const size_t HW = static_cast<size_t>(a.H) * a.W, rs = 3 * static_cast<size_t>(a.C);
  const uint32_t rsb = static_cast<uint32_t>(rs) * 2u, nrec = static_cast<uint32_t>(HW - 1) * rsb + D * 2u;
  const uint32_t lds0 = lds_base(smem);
  const char *kb = smem, *vb = smem + TILE;
  const float *s_dsf = reinterpret_cast<const float *>(s_ds);

  // the relative offset this thread sums: tid = (ry + K - 1) (2 K - 1) + rx + K - 1, key - query
  const int ry = tid / (2 * K - 1) - (K - 1), rx = tid % (2 * K - 1) - (K - 1);
  float gsum = 0.f;
  if (tid < G::R) s_bias[tid] = bias[h * G::R + tid] * LOG2E;

  const long it1 = (run + 1) * a.per < a.items ? (run + 1) * a.per : a.items;
  for (long it = run * a.per; it < it1; ++it) {
    const Patch p = patch_of(it, a);
    const int hy0 = nb<K>(p.y0, a.H), hx0 = nb<K>(p.x0, a.W);
    const bf16_t *base = qkv + static_cast<size_t>(p.b) * HW * rs + h * D;
    stage_halo<HS, G::NR>(make_rsrc(base + a.C, nrec), rsb, make_rsrc(base + 2 * a.C, nrec), rsb, lds0, hy0, hx0, a.H,
                          a.W, wave, lane);
    const Query<K> q(p, hy0, hx0, wave, i, a);
    const size_t pix = static_cast<size_t>(q.y) * a.W + q.x;
    const size_t st = (static_cast<size_t>(p.b) * a.nhead + h) * HW + pix;
    bf16x8 qf[1], gf[1];
    load_row<1>(base + pix * rs, q.ok, g, qf);
    load_row<1>(dout + (static_cast<size_t>(p.b) * HW + pix) * a.C + h * D, q.ok, g, gf);
    const float l2 = q.ok ? lse2[st] : 0.f;
    wait_vmcnt<0>();
    __syncthreads();  // the halo is in LDS

    if (p.y0 + 2 * wave < a.H) {
      const int n0 = q.kb0 + 4 * g;
      f32x4 ps[NKT], dp[NKT];
      float dsl = 0.f;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        ps[kt] = mma(row_frag(kb, q.kb0 + 16 * kt + i, g), qf[0], zero4());
        dp[kt] = mma(row_frag(vb, q.kb0 + 16 * kt + i, g), gf[0], zero4());
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          int idx;
          const bool on = q.pair(n0 + 16 * kt + j, idx);
          const float v = mul_rn(ps[kt][j], a.sc2) + s_bias[idx];
          ps[kt][j] = on ? __builtin_amdgcn_exp2f(v - l2) : 0.f;
          dsl = fmaf(ps[kt][j], dp[kt][j], dsl);
        }
      }
      dsl += __shfl_xor(dsl, 16, 64);
      dsl += __shfl_xor(dsl, 32, 64);
      if (g == 0 && q.ok) dsum[st] = dsl;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) ps[kt][j] *= dp[kt][j] - dsl;  // dS
        s_ds[(wave * NKT + kt) * 64 + lane] = ps[kt];
      }
      if (dq) {
        f32x4 acc[2] = {zero4(), zero4()};
#pragma unroll
        for (int kp = 0; kp < (NKT + 1) / 2; ++kp) {
          const bf16x8 df = pack_frag(ps[2 * kp], 2 * kp + 1 < NKT ? ps[2 * kp + 1 < NKT ? 2 * kp + 1 : 0] : zero4());
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) acc[dt] = mma(tr_frag(kb, q.kb0 + 32 * kp, dt, i, g), df, acc[dt]);
        }
        if (q.ok) store_row<2>(dq + (static_cast<size_t>(p.b) * HW + pix) * dqs + h * D, g, acc, a.scale);
      }
    }
    __syncthreads();  // the fp32 dS is in LDS

    if (tid < G::R) {  // over the patch's queries in order: dS[query][key = query + (ry, rx)]
      float sum = 0.f;
      for (int t = 0; t < PS * PS; ++t) {
        const int qy = t >> 3, qx = t & 7, y = p.y0 + qy, x = p.x0 + qx, w = qy >> 1;
        const int ky = y + ry, kx = x + rx;
        const bool in = y < a.H && x < a.W &&
                        static_cast<unsigned>(ky - nb<K>(y, a.H)) < static_cast<unsigned>(K) &&
                        static_cast<unsigned>(kx - nb<K>(x, a.W)) < static_cast<unsigned>(K);
        // the key's place among the wave's tile rows, then the lane and slot that held it
        const int kl = (ky - nb<K>(p.y0 + 2 * w, a.H)) * HS + kx - hx0;
        const int e = (((w * NKT + (kl >> 4)) * 64 + ((kl >> 2) & 3) * 16 + (qy & 1) * 8 + qx) << 2) + (kl & 3);
        const float v = s_dsf[in ? e : 0];
        sum += in ? v : 0.f;
      }
      gsum += sum;
    }
    __syncthreads();  // every reader of the halo and of dS is done: the next item may land
  }
  if (tid < G::R) slabs[static_cast<size_t>(blockIdx.x) * G::R + tid] = gsum;
}

// ----------------------------------------------------------------- backward, key orientation
// One block per (sample, patch, head): dK and dV of the patch's pixels into dqkv (which may be qkv).
template <int K>
__global__ __launch_bounds__(NT) void nattn_bwd_kv(const bf16_t *qkv, const bf16_t *__restrict__ dout,
                                                   const float *__restrict__ bias, const float *__restrict__ lse2,
                                                   const float *__restrict__ dsum, bf16_t *dqkv, const NArgs a) {
  using G = Geo<K>;
  constexpr int QS = G::QS, NRQ = G::NRQ, TILE = NRQ * D * 2;
  __shared__ __attribute__((aligned(1024))) char smem[2 * TILE];  // Q | dO
  __shared__ float s_l2[NRQ], s_dd[NRQ], s_bias[G::R + 7];        // lse2 and D of the staged queries
  __shared__ int s_yx[NRQ];                                       // their pixel y << 16 | x, -1: none
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int h = blockIdx.x % a.nhead;
  const Patch p = patch_of(blockIdx.x / a.nhead, a);
  const int ymin = lo_q<K>(p.y0), xmin = lo_q<K>(p.x0);
  const size_t HW = static_cast<size_t>(a.H) * a.W, rs = 3 * static_cast<size_t>(a.C);
  const bf16_t *base = qkv + static_cast<size_t>(p.b) * HW * rs + h * D;
  const bf16_t *gbase = dout + static_cast<size_t>(p.b) * HW * a.C + h * D;
  const uint32_t rsb = static_cast<uint32_t>(rs) * 2u, gsb = static_cast<uint32_t>(a.C) * 2u;
  const uint32_t nrec = static_cast<uint32_t>(HW - 1) * rsb + D * 2u, grec = static_cast<uint32_t>(HW - 1) * gsb + D * 2u;

  stage_halo<QS, NRQ>(make_rsrc(base, nrec), rsb, make_rsrc(gbase, grec), gsb, lds_base(smem), ymin, xmin, a.H, a.W,
                      wave, lane);
  {
    const size_t st = (static_cast<size_t>(p.b) * a.nhead + h) * HW;
    for (int n = tid; n < NRQ; n += NT) {
      const int hy = n / QS, hx = n - hy * QS, y = ymin + hy, x = xmin + hx;
      const bool ok = hy < QS && y < a.H && x < a.W;
      const size_t e = st + (ok ? static_cast<size_t>(y) * a.W + x : 0);
      s_yx[n] = ok ? (y << 16) | x : -1;
      s_l2[n] = ok ? lse2[e] : 0.f;
      s_dd[n] = ok ? dsum[e] : 0.f;
    }
    if (tid < G::R) s_bias[tid] = bias[h * G::R + tid] * LOG2E;
  }
  const int yk0 = p.y0 + 2 * wave;
  const int yk = yk0 + (i >> 3), xk = p.x0 + (i & 7);
  const bool okk = yk < a.H && xk < a.W;
  const size_t pix = static_cast<size_t>(yk) * a.W + xk;
  bf16x8 kf[1], vf[1];
  load_row<1>(base + pix * rs + a.C, okk, g, kf);
  load_row<1>(base + pix * rs + 2 * a.C, okk, g, vf);
  wait_vmcnt<0>();
  __syncthreads();
  if (yk0 >= a.H) return;  // (no barrier follows)

  const char *qb = smem, *gb = smem + TILE;
  // the halo rows that attend the wave's two key rows, and their 32-query steps
  const int wmin = lo_q<K>(yk0), wmax = hi_q<K>(min(yk0 + 1, a.H - 1), a.H);
  const int qb0 = (wmin - ymin) * QS, npair = ((wmax - wmin + 1) * QS + 31) >> 5;
  f32x4 dk[2] = {zero4(), zero4()}, dv[2] = {zero4(), zero4()};
  for (int qp = 0; qp < npair; ++qp) {
    f32x4 ps[2], ds[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int r0 = qb0 + 32 * qp + 16 * t;
      ps[t] = mma(row_frag(qb, r0 + i, g), kf[0], zero4());
      ds[t] = mma(row_frag(gb, r0 + i, g), vf[0], zero4());
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = r0 + 4 * g + j, yx = s_yx[n], y = yx >> 16, x = yx & 0xffff;
        const bool on = okk && yx >= 0 &&
                        static_cast<unsigned>(yk - nb<K>(y, a.H)) < static_cast<unsigned>(K) &&
                        static_cast<unsigned>(xk - nb<K>(x, a.W)) < static_cast<unsigned>(K);
        const int idx = on ? (yk - y + K - 1) * (2 * K - 1) + xk - x + K - 1 : 0;
        const float v = mul_rn(ps[t][j], a.sc2) + s_bias[idx];
        ps[t][j] = on ? __builtin_amdgcn_exp2f(v - s_l2[n]) : 0.f;
        ds[t][j] = on ? ps[t][j] * (ds[t][j] - s_dd[n]) : 0.f;
      }
    }
    const bf16x8 pf = pack_frag(ps[0], ps[1]), df = pack_frag(ds[0], ds[1]);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      dv[dt] = mma(tr_frag(gb, qb0 + 32 * qp, dt, i, g), pf, dv[dt]);
      dk[dt] = mma(tr_frag(qb, qb0 + 32 * qp, dt, i, g), df, dk[dt]);
    }
  }
  if (okk) {
    bf16_t *orow = dqkv + (static_cast<size_t>(p.b) * HW + pix) * rs + h * D;
    store_row<2>(orow + a.C, g, dk, a.scale);
    store_row<2>(orow + 2 * a.C, g, dv, 1.f);
  }
}

// gbias[h][r] += sum over the runs of slab (run, h)[r], in run order
__global__ __launch_bounds__(NT) void nattn_merge(const float *__restrict__ slabs, int runs, int n, float *gbias) {
  const int e = blockIdx.x * NT + threadIdx.x;  // h R + r
  if (e >= n) return;
  float sum = 0.f;
  for (int p = 0; p < runs; ++p) sum += slabs[static_cast<size_t>(p) * n + e];
  gbias[e] += sum;
}

// dqkv [rows][3 C] columns 0 .. C - 1 = stage [rows][C], 16 bytes per thread; cu = C / 8
__global__ __launch_bounds__(NT) void nattn_copy_dq(const uint4 *__restrict__ stage, uint4 *__restrict__ dqkv, long n,
                                                    int cu) {
  const long e = static_cast<long>(blockIdx.x) * NT + threadIdx.x;
  if (e >= n) return;
  const long r = e / cu;
  dqkv[r * 3 * cu + (e - r * cu)] = stage[e];
}

// false: the kernels do not serve the shape
static bool make_args(NArgs &a, long B, int H, int W, int C, int nhead, int k) {
  if (B < 1 || nhead < 1 || C != nhead * D || !(k == 3 || k == 5 || k == 7)) return false;
  if (H < k || W < k || H > 0x7fff || W > 0x7fff) return false;
  if (static_cast<long>(H) * W * 3 * C * 2 > 0x7fffffffL) return false;  // (32-bit row offsets per sample)
  a.H = H, a.W = W, a.C = C, a.nhead = nhead;
  a.npx = (W + PS - 1) / PS;
  a.npatch = (H + PS - 1) / PS * a.npx;
  a.items = B * a.npatch;
  if (a.items * nhead > 0x7fffffffL || B * H * W * (C / 8) > 0x7fffffffL * NT) return false;
  // the query orientation's cut: at most PMAX / nhead runs of equal length, a function of the shape alone
  const long cap = PMAX / nhead > 1 ? PMAX / nhead : 1;
  a.per = (a.items + cap - 1) / cap;
  a.scale = 0.17677669529663687f;
  a.sc2 = a.scale * LOG2E;
  return true;
}

static long runs_of(const NArgs &a) { return (a.items + a.per - 1) / a.per; }

}  // namespace

// fp32 workspace of cxn_nattn_bwd for every batch 1 .. B: one slab of (2 k - 1)^2 floats per (run,
// head).  The run count is not monotone in the batch (items 3136 at a cap of 384 cut into 349 runs
// of 9, items 2303 into 384 runs of 6), so this is its ceiling min(items, cap), which only grows
// with B.  0: shape not served
CXN_API long cxn_nattn_ws_floats(long B, int H, int W, int C, int nhead, int kernel) {
  NArgs a;
  if (!make_args(a, B, H, W, C, nhead, kernel)) return 0;
  const long cap = PMAX / nhead > 1 ? PMAX / nhead : 1;
  return (a.items < cap ? a.items : cap) * nhead * (2 * kernel - 1) * (2 * kernel - 1);
}

#define NATTN_BY_K(KER, ...)                          \
  switch (kernel) {                                   \
    case 3: CXN_LAUNCH((KER<3>), __VA_ARGS__); break; \
    case 5: CXN_LAUNCH((KER<5>), __VA_ARGS__); break; \
    default: CXN_LAUNCH((KER<7>), __VA_ARGS__);       \
  }

// out [B H W][C] = softmax over the clamped kernel x kernel neighbourhood of (q k^T / sqrt(d) + bias) v
// of qkv [B H W][3 C]; bias [nhead][(2 kernel - 1)^2] fp32; lse and lse2 [B nhead H W] fp32 receive
// every row's log-sum-exp in natural and in the kernel's log2 units.  out must not alias qkv.
CXN_API int cxn_nattn_fwd(const void *qkv, void *out, const float *bias, float *lse, float *lse2, long B, int H,
                          int W, int C, int nhead, int kernel, void *stream) {
  NArgs a;
  if (!qkv || !out || !bias || !lse || !lse2 || qkv == out || !make_args(a, B, H, W, C, nhead, kernel) ||
      !(aligned16(qkv) && aligned16(out)))
    return -1;
  const int grid = static_cast<int>(a.items * nhead);
  NATTN_BY_K(nattn_fwd, grid, NT, 0, S_, static_cast<const bf16_t *>(qkv), static_cast<bf16_t *>(out), bias, lse, lse2,
             a);
  RET;
}

// gbias [nhead][(2 kernel - 1)^2] += the bias gradient; dqkv (nullable: parameter gradient only) =
// the gradient of qkv given dout [B H W][C] and the forward's lse2; dsum [B nhead H W] receives D.
// dqkv may be qkv, and then dq_stage [B H W][C] bf16 is required (dQ passes through it); otherwise it
// is not touched and may be null.  slabs: fp32 workspace of ws_floats >= cxn_nattn_ws_floats(..);
// -2 when it is smaller.
CXN_API int cxn_nattn_bwd(const void *qkv, const void *dout, const float *bias, const float *lse2, float *dsum,
                          void *dqkv, void *dq_stage, float *gbias, float *slabs, long ws_floats, long B, int H, int W,
                          int C, int nhead, int kernel, void *stream) {
  NArgs a;
  if (!qkv || !dout || !bias || !lse2 || !dsum || !gbias || dout == dqkv || dout == dq_stage || qkv == dq_stage ||
      (dqkv == qkv && !dq_stage) || !make_args(a, B, H, W, C, nhead, kernel) ||
      !(aligned16(qkv) && aligned16(dout) && aligned16(dqkv) && aligned16(dq_stage)))
    return -1;
  const int runs = static_cast<int>(runs_of(a)), n = nhead * (2 * kernel - 1) * (2 * kernel - 1);
  if (!slabs || static_cast<long>(runs) * n > ws_floats) return -2;
  const bool in_place = dqkv == qkv;
  bf16_t *dq = static_cast<bf16_t *>(in_place ? dq_stage : dqkv);
  const long dqs = in_place ? C : 3L * C;
  NATTN_BY_K(nattn_bwd_q, runs * nhead, NT, 0, S_, static_cast<const bf16_t *>(qkv), static_cast<const bf16_t *>(dout),
             bias, lse2, dsum, dq, dqs, slabs, a);
  CXN_LAUNCH((nattn_merge), (n + NT - 1) / NT, NT, 0, S_, (const float *)slabs, runs, n, gbias);
  if (dqkv) {
    const int grid = static_cast<int>(a.items * nhead);
    NATTN_BY_K(nattn_bwd_kv, grid, NT, 0, S_, static_cast<const bf16_t *>(qkv), static_cast<const bf16_t *>(dout), bias,
               lse2, (const float *)dsum, static_cast<bf16_t *>(dqkv), a);
    if (in_place) {
      const long units = B * H * W * (C / 8);
      CXN_LAUNCH((nattn_copy_dq), static_cast<int>((units + NT - 1) / NT), NT, 0, S_, (const uint4 *)dq_stage,
                 static_cast<uint4 *>(dqkv), units, C / 8);
    }
  }
  RET;
}
