// reductions: column sums of [rows][C] matrices (the bias gradients, reference K5/K11) and the sums
// over split-K slabs, with the process-wide switches that choose how they combine partial sums.
//
//   cxn_set_deterministic     ordered passes instead of atomics wherever the order would vary
//   cxn_set_kernel_variant    A/B switches of single kernels (nn_shared.h)
//   nn::reduce_partials       db += the partial rows another kernel left in a workspace
//   cxn_colsum                db += column sums of one bf16 matrix
//   cxn_colsum_multi          every deferred bias gradient of a backward pass in one launch
//   cxn_splitk_accumulate     out += split-K slabs in slice order (fp32)
//   cxn_splitk_finalize(_dropout)  bf16 out = epilogue(sum of slabs): bias, relu, mask, dropout
//
// Return 0, a negative code for a shape or workspace they cannot serve, or -3 when a launch failed.
#include "nn_shared.h"

int cxn_deterministic = 0;
CXN_API int cxn_set_deterministic(int on) {
  cxn_deterministic = on ? 1 : 0;
  return 0;
}

int nn::colsum_split = 1;  // cxn_set_kernel_variant(1, v): 0 keeps colsum_multi's whole-row blocks (A/B)
CXN_API int cxn_set_kernel_variant(int which, int v) {
  if (which == 0) nn::pool_cells = v;
  else if (which == 1) nn::colsum_split = v;
  else return -1;
  return 0;
}

namespace {
// db[c] += sum_b part[b][c].  Block = 32 columns x 8 row groups over one chunk of rows
// (blockIdx.y); one atomic per column per chunk (a few dozen per address).
__global__ void partials_reduce(const float *__restrict__ part, int nb, int C, float *__restrict__ db) {
  const int c = blockIdx.x * 32 + (threadIdx.x & 31);
  const int rg = threadIdx.x >> 5;
  const int per = (nb + gridDim.y - 1) / gridDim.y;
  const int b0 = blockIdx.y * per, b1 = min(nb, b0 + per);
  float s = 0.f;
  if (c < C) {
#pragma unroll 4
    for (int b = b0 + rg; b < b1; b += 8) s += part[static_cast<long>(b) * C + c];
  }
  __shared__ float red[8][33];
  red[rg][threadIdx.x & 31] = s;
  __syncthreads();
  if (rg == 0 && c < C) {
    float t = 0.f;
#pragma unroll
    for (int g = 0; g < 8; ++g) t += red[g][threadIdx.x & 31];
    atomicAdd(db + c, t);
  }
}
}  // namespace

void nn::reduce_partials(const float *ws, int nb, int C, float *db, void *stream) {
  // one row chunk (a single fixed-order pass, one add per column) in deterministic mode
  const dim3 grid((C + 31) / 32, cxn_deterministic ? 1 : (nb + 63) / 64);
  CXN_LAUNCH((partials_reduce), grid, NT, 0, S_, ws, nb, C, db);
}

namespace {
// db[c] += sum_r dy[r][c]  (dy bf16 [rows][C], C % 8 == 0).  Block = CB column-vectors x RG row
// groups; per-thread fp32 partials, LDS tree over RG, then one fp32 atomic per channel per block
// into db (one launch), or, in deterministic mode (db == nullptr), one partial row per block
// for the fixed-order partials_reduce.
__global__ void colsum_bf16(const bf16_t *__restrict__ dy, float *__restrict__ part, long rows, int C,
                            int rows_per_block, float *__restrict__ db) {
  const int CV = C / 8;
  const int CB = min(CV - static_cast<int>(blockIdx.y) * 64, 64);
  const int RG = NT / CB;
  const int t = threadIdx.x;
  const int cvl = t % CB, rg = t / CB;
  const int cv = blockIdx.y * 64 + cvl;
  const long r0 = static_cast<long>(blockIdx.x) * rows_per_block;
  const long r1 = min(rows, r0 + rows_per_block);
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (rg < RG) {
    constexpr int U = 4;  // independent 16-B loads in flight per thread
    for (long r = r0 + rg; r < r1; r += RG * U) {
      uint4 q[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long rr = r + static_cast<long>(u) * RG;
        q[u] = rr < r1 ? *reinterpret_cast<const uint4 *>(dy + rr * C + cv * 8) : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float v[8];
        unpack8(q[u], v);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += v[e];
      }
    }
  }
  __shared__ float red[NT][9];
#pragma unroll
  for (int e = 0; e < 8; ++e) red[t][e] = (rg < RG) ? acc[e] : 0.f;
  __syncthreads();
  for (int q = t; q < CB * 8; q += NT) {
    const int c = q / 8, e = q % 8;
    float s = 0.f;
    for (int g = 0; g < RG; ++g) s += red[g * CB + c][e];
    if (db != nullptr)
      atomicAdd(db + (blockIdx.y * 64 + c) * 8 + e, s);
    else
      part[static_cast<long>(blockIdx.x) * C + (blockIdx.y * 64 + c) * 8 + e] = s;  // reduced by partials_reduce
  }
}

// Small / ragged C: one thread per column.
__global__ void colsum_scalar(const bf16_t *__restrict__ dy, float *__restrict__ db, long rows, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (long r = 0; r < rows; ++r) s += bf2f(dy[r * C + c]);
  db[c] += s;
}
}  // namespace

CXN_API int cxn_colsum(const void *dy, float *db, long rows, int C, float *ws, long ws_elems, void *stream) {
  if (C % 8) {
    CXN_LAUNCH((colsum_scalar), cdiv(C, NT), NT, 0, S_, (const bf16_t *)dy, db, rows, C);
    RET;
  }
  const int CV = C / 8;
  int rpb = 512;
  // keep the partials within the caller's workspace
  while (static_cast<long>(cdiv(rows, rpb)) * C > ws_elems && rpb < (1 << 24)) rpb *= 2;
  // atomics straight into db: at most ~512 adders per channel (VGG conv1_2's 3.2M rows at 512
  // rows per block put 6272 atomics on each of 64 addresses and ran slower than two passes)
  if (!cxn_deterministic)
    while (cdiv(rows, rpb) > 512) rpb *= 2;
  if (static_cast<long>(cdiv(rows, rpb)) * C > ws_elems) return -2;
  dim3 grid(cdiv(rows, rpb), cdiv(CV, 64));
  if (!cxn_deterministic) {  // per-block atomics straight into db
    CXN_LAUNCH((colsum_bf16), grid, NT, 0, S_, (const bf16_t *)dy, ws, rows, C, rpb, db);
    RET;
  }
  CXN_LAUNCH((colsum_bf16), grid, NT, 0, S_, (const bf16_t *)dy, ws, rows, C, rpb, nullptr);
  nn::reduce_partials(ws, static_cast<int>(grid.x), C, db, stream);
  RET;
}

namespace {
// Every deferred bias gradient of a backward pass in one launch (blockIdx.y = segment):
// db_s[c] += sum_r dy_s[r][c], C_s % 8 == 0, per-block partials -> one atomic per channel.
// A layer's backward only queues its (dy, db); NeuralNet.backprop flushes the queue once at
// the end (dy buffers are not rewritten later in the pass), which replaces one or two small
// launches per conv / fc layer -- GoogLeNet has 57 -- by one.
// A masked segment sums a max-pool's OUTPUT gradient instead of the conv's: every pool window
// routes its gradient to exactly one input pixel, and relu' of that pixel is bit 7 of the
// window's recorded offset (pool_fwd_rows, relu & 2), so sum_pixels dx = sum_windows dy * relu'
// -- the bias gradient of the conv in front of a max-pool at 1/stride^2 of the bytes read.
constexpr int COLSUM_MAXSEG = 64;
struct ColsumSeg {
  const bf16_t *dy;
  const uint8_t *mask;  // nullable: max-pool offsets [rows][C]; entries with bit 7 set count as 0
  float *db;
  long rows;
  long ld;  // dy row stride in elements (>= C: a channel slice of a wider NHWC buffer); mask rows are C
  int C, rpb, nblk, nchunk;
};
struct ColsumTable {
  ColsumSeg s[COLSUM_MAXSEG];
  int b0[COLSUM_MAXSEG];  // first block of each segment on the flat grid
  int n;
};
__global__ void colsum_multi(ColsumTable tab) {
  // flat grid, blocks split over segments by size (a 2-D grid of max-blocks x segments would
  // launch tens of thousands of idle blocks for GoogLeNet's 57 segments)
  const int bx = blockIdx.x;
  int si = 0;
  for (int i = 1; i < tab.n; ++i)
    if (tab.b0[i] <= bx) si = i;
  const ColsumSeg sg = tab.s[si];
  const int blk = bx - tab.b0[si];
  const int CV = sg.C / 8;
  const int t = threadIdx.x;
  // nchunk > 1: each block owns one chunk of 64 column vectors (wide fc segments would
  // otherwise leave one block walking all 4096 columns); 1: the block walks every chunk
  const int rb = blk / sg.nchunk, chunk = blk - rb * sg.nchunk;
  const int cbeg = sg.nchunk > 1 ? chunk * 64 : 0, cend = sg.nchunk > 1 ? min(CV, cbeg + 64) : CV;
  const long r0 = static_cast<long>(rb) * sg.rpb;
  const long r1 = min(sg.rows, r0 + sg.rpb);
  __shared__ float red[NT][9];
  for (int cb = cbeg; cb < cend; cb += 64) {
    const int CB = min(cend - cb, 64);
    const int RG = NT / CB;
    const int cvl = t % CB, rg = t / CB;
    const int cv = cb + cvl;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rg < RG) {
      // 8 rows in flight per thread; whole groups of 8 without bounds checks
      constexpr int U = 8;
      const long e0 = (r0 + rg) * sg.C + cv * 8;
      const bf16_t *p = sg.dy + (r0 + rg) * sg.ld + cv * 8;
      const long step = static_cast<long>(RG) * sg.ld;  // masked segments have ld == C
      long r = r0 + rg;
      if (sg.mask == nullptr) {
        for (; r + (U - 1) * RG < r1; r += RG * U, p += U * step) {
          uint4 q[U];
#pragma unroll
          for (int u = 0; u < U; ++u) q[u] = *reinterpret_cast<const uint4 *>(p + u * step);
#pragma unroll
          for (int u = 0; u < U; ++u) {
            float v[8];
            unpack8(q[u], v);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += v[e];
          }
        }
        for (; r < r1; r += RG, p += step) {
          float v[8];
          unpack8(*reinterpret_cast<const uint4 *>(p), v);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] += v[e];
        }
      } else {
        const uint8_t *mp = sg.mask + e0;
        auto add = [&](const uint4 q, const uint2 m) {
          float v[8];
          unpack8(q, v);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[e] += ((m.x >> (8 * e + 7)) & 1u) ? 0.f : v[e];
            acc[e + 4] += ((m.y >> (8 * e + 7)) & 1u) ? 0.f : v[e + 4];
          }
        };
        for (; r + (U - 1) * RG < r1; r += RG * U, p += U * step, mp += U * step) {
          uint4 q[U];
          uint2 m[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            q[u] = *reinterpret_cast<const uint4 *>(p + u * step);
            m[u] = *reinterpret_cast<const uint2 *>(mp + u * step);
          }
#pragma unroll
          for (int u = 0; u < U; ++u) add(q[u], m[u]);
        }
        for (; r < r1; r += RG, p += step, mp += step)
          add(*reinterpret_cast<const uint4 *>(p), *reinterpret_cast<const uint2 *>(mp));
      }
    }
    __syncthreads();  // red is reused by the next column chunk
#pragma unroll
    for (int e = 0; e < 8; ++e) red[t][e] = (rg < RG) ? acc[e] : 0.f;
    __syncthreads();
    for (int q = t; q < CB * 8; q += NT) {
      const int c = q / 8, e = q % 8;
      float sum = 0.f;
      for (int gq = 0; gq < RG; ++gq) sum += red[gq * CB + c][e];
      atomicAdd(sg.db + (cb + c) * 8 + e, sum);
    }
  }
}
}  // namespace

// dys / dbs / rows / Cs: n deferred bias gradients (C % 8 == 0 each); masks: nullable array of
// nullable max-pool offset tensors (masked segments, see colsum_multi)
CXN_API int cxn_colsum_multi(const void *const *dys, float *const *dbs, const long *rows, const int *Cs,
                             const void *const *masks, int n, void *stream, const long *lds) {
  for (int base = 0; base < n; base += COLSUM_MAXSEG) {
    ColsumTable tab;
    const int cnt = n - base < COLSUM_MAXSEG ? n - base : COLSUM_MAXSEG;
    int nblk = 0;
    tab.n = cnt;
    for (int i = 0; i < cnt; ++i) {
      const int j = base + i;
      if (Cs[j] % 8) return -1;
      const long ld = lds ? lds[j] : Cs[j];
      if (ld % 8 || ld < Cs[j] || (masks && masks[j] && ld != Cs[j])) return -1;
      // <= 1024 blocks (adders per channel) per segment, >= 256 rows per block: the largest
      // segment (AlexNet conv1: 774k rows) needs ~4 blocks per CU to keep HBM busy
      long nb = cdiv(rows[j], 256L);
      int nchunk = 1;
      if (nn::colsum_split) {
        // one block per (rows, chunk of <= 64 column vectors) reading ~96 KiB, >= 8 rows per
        // thread (one round of the 8-deep load batch): fc6 (256 x 4096) gets 24 blocks, not 1
        const int CV = Cs[j] / 8;
        nchunk = (CV + 63) / 64;
        const int CB = CV < 64 ? CV : 64;
        const long bpr = static_cast<long>(CB) * 8 * (masks && masks[j] ? 3 : 2);
        long want = 98304 / bpr;
        const long minr = (NT / CB) * 8L;
        if (want < minr) want = minr;
        nb = cdiv(rows[j], want);
      }
      if (nb > 1024) nb = 1024;
      if (nb < 1) nb = 1;
      const int rpb = rows[j] > 0 ? static_cast<int>(cdiv(rows[j], nb)) : 1;
      const int nrb = static_cast<int>(cdiv(rows[j], static_cast<long>(rpb)));
      tab.s[i] = ColsumSeg{static_cast<const bf16_t *>(dys[j]),
                           masks ? static_cast<const uint8_t *>(masks[j]) : nullptr, dbs[j], rows[j], ld, Cs[j], rpb,
                           nrb * nchunk, nchunk};
      tab.b0[i] = nblk;
      nblk += tab.s[i].nblk;
    }
    if (nblk > 0) CXN_LAUNCH((colsum_multi), nblk, NT, 0, S_, tab);
  }
  RET;
}

namespace {
// out[i] += sum_s ws[s][i], slabs summed in slice order: the deterministic replacement for
// split-K fp32 atomics (conv weight-grad in deterministic mode).
__global__ void splitk_accumulate(const float *__restrict__ ws, int nsplit, long slab, float *__restrict__ out) {
  for (long i = (static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x) * 4; i < slab;
       i += static_cast<long>(gridDim.x) * blockDim.x * 4) {
    if (i + 4 <= slab) {
      f32x4 acc = *reinterpret_cast<const f32x4 *>(out + i);
      for (int s = 0; s < nsplit; ++s) acc += *reinterpret_cast<const f32x4 *>(ws + s * slab + i);
      *reinterpret_cast<f32x4 *>(out + i) = acc;
    } else {
      for (long e = i; e < slab; ++e) {
        float a = out[e];
        for (int s = 0; s < nsplit; ++s) a += ws[s * slab + e];
        out[e] = a;
      }
    }
  }
}
}  // namespace

CXN_API int cxn_splitk_accumulate(const float *ws, int nsplit, long slab, float *out, void *stream) {
  if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(out)) & 15 || slab % 4) return -1;
  long b = (slab / 4 + NT - 1) / NT;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  CXN_LAUNCH((splitk_accumulate), static_cast<int>(b), NT, 0, S_, ws, nsplit, slab, out);
  RET;
}

namespace {
// Split-K finalisation: out[r][c] = epilogue(sum_s ws[s][r][c]) with optional bias[c],
// relu, and mask_relu (keep where the OLD out value is > 0).  8 columns per thread.

// DROP: the dropout layer behind a fused fc -> relu is applied here as well (keep iff
// hash(seed, flat index) < thresh, kept values * scale), with dropout_apply's mask
template <bool DROP>
__global__ void splitk_finalize(const float *__restrict__ ws, int nsplit, long slab, bf16_t *out, long rows,
                                int cols, const float *__restrict__ bias, int relu, int mask_relu, uint32_t seed0,
                                const int *counter, uint32_t thresh, float scale) {
  // grid: blockIdx.y = row, x over 8-column groups (no 64-bit division per element)
  {
    const long r = blockIdx.y;
    const int c0 = (blockIdx.x * blockDim.x + threadIdx.x) * 8;
    if (c0 >= cols) return;
    const float *p = ws + r * cols + c0;
    float f[8];
    {
      const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
      f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    }
    for (int sidx = 1; sidx < nsplit; ++sidx) {
      const float4 a = *reinterpret_cast<const float4 *>(p + sidx * slab);
      const float4 b = *reinterpret_cast<const float4 *>(p + sidx * slab + 4);
      f[0] += a.x; f[1] += a.y; f[2] += a.z; f[3] += a.w; f[4] += b.x; f[5] += b.y; f[6] += b.z; f[7] += b.w;
    }
    bf16_t *dst = out + r * cols + c0;
    float old[8];
    if (mask_relu) unpack8(*reinterpret_cast<const uint4 *>(dst), old);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (bias) f[e] += bias[c0 + e];
      if (relu) f[e] = fmaxf(f[e], 0.f);
      if (mask_relu && !(old[e] > 0.f)) f[e] = 0.f;
    }
    if constexpr (DROP) {
      const uint32_t seed = counter ? hash_u32(static_cast<uint32_t>(*counter), seed0) : seed0;
      const uint32_t i0 = static_cast<uint32_t>(r * cols + c0);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = hash_u32(i0 + e, seed) < thresh ? f[e] * scale : 0.f;
    }
    *reinterpret_cast<uint4 *>(dst) = pack8(f);
  }
}
}  // namespace

CXN_API int cxn_splitk_finalize(const float *ws, int nsplit, long slab, void *out, long rows, int cols,
                                const float *bias, int relu, int mask_relu, void *stream) {
  if (cols % 8) return -2;
  dim3 grid(cdiv(cols / 8, NT), static_cast<unsigned>(rows));
  CXN_LAUNCH((splitk_finalize<false>), grid, NT, 0, S_, ws, nsplit, slab, (bf16_t *)out, rows, cols, bias, relu,
             mask_relu, 0u, (const int *)nullptr, 0u, 1.f);
  RET;
}
// the same with the dropout of a fused fc -> relu -> dropout (mask as cxn_dropout)
CXN_API int cxn_splitk_finalize_dropout(const float *ws, int nsplit, long slab, void *out, long rows, int cols,
                                        const float *bias, int relu, unsigned seed, const int *counter, float pkeep,
                                        void *stream) {
  if (cols % 8 || static_cast<double>(rows) * cols >= 4294967296.0) return -2;
  dim3 grid(cdiv(cols / 8, NT), static_cast<unsigned>(rows));
  CXN_LAUNCH((splitk_finalize<true>), grid, NT, 0, S_, ws, nsplit, slab, (bf16_t *)out, rows, cols, bias, relu, 0,
             static_cast<uint32_t>(seed), counter, dropout_thresh(pkeep), 1.f / pkeep);
  RET;
}
