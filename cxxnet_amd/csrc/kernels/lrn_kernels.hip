// lrn: cross-channel local response normalisation on NHWC bf16 (reference
// src/layer/lrn_layer-inl.hpp:53-74), alone and fused with the 3x3 / 2 max pool in front of it.
//
//   cxn_lrn_fwd        y = x * norm^-beta, norm[c] = knorm + alpha / n * sum of x^2 over the window
//   cxn_lrn_bwd        dx; norm is recomputed from x, no state tensor is stored
//   cxn_lrn_bwd_db     cxn_lrn_bwd plus db += column sums of the stored dx
//   cxn_pool_lrn_fwd   max pool -> LRN in one pass (pooled P, offsets and Y)
//   cxn_lrn_pool_bwd   LRN -> max pool backward: the pooled gradient never reaches HBM
//
// C % 8 == 0 throughout.  The shuffle forms (C / 8 <= 64 lanes per pixel, local_size <= 9) keep the
// window sums in registers; the launchers return -1 for a shape they do not serve, with nothing
// launched, and -3 when a launch failed.
#include "nn_shared.h"

namespace {
// The norm's powers: norm = k + alpha / n * sum(x^2) >= k > 0 (k = 1 in every shipped net), so the
// raw v_log_f32 / v_exp_f32 give exp2f / __log2f's values without their denormal-range fix-ups
// (a compare, a select and a scale per call: a third of the fused pool -> LRN backward's VALU).
__device__ __forceinline__ float lrn_log2(float x) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float lrn_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
// norm[c] = knorm + alpha/n * sum_{c' in [c-h, c+h] clipped} x[c']^2 ; y = x * norm^-beta
// One thread per (pixel, 8 channels); halo of up to 8 channels each side via three 16-B loads.
__device__ __forceinline__ void load_window(const bf16_t *row, int C, int c0, float *buf /*[24]*/) {
  // buf[j] = x[c0 - 8 + j], zero outside [0, C)
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const int cs = c0 - 8 + 8 * b;
    float v[8];
    if (cs >= 0 && cs + 8 <= C) {
      unpack8(*reinterpret_cast<const uint4 *>(row + cs), v);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (cs + e >= 0 && cs + e < C) ? bf2f(row[cs + e]) : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) buf[8 * b + e] = v[e];
  }
}

__global__ void lrn_fwd(const bf16_t *__restrict__ x, bf16_t *__restrict__ y, long npix, int C, int half,
                        float salpha, float beta, float knorm) {
  const int CV = C / 8;
  const long total = npix * CV;
  for (long idx = grid_stride_start(); idx < total; idx += grid_stride()) {
    const long pix = idx / CV;
    const int c0 = (idx % CV) * 8;
    const bf16_t *row = x + pix * C;
    float xb[24];
    load_window(row, C, c0, xb);
    float out[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float s = 0.f;
      for (int d = -half; d <= half; ++d) {
        const float v = xb[8 + e + d];
        s += v * v;
      }
      const float norm = knorm + salpha * s;
      out[e] = xb[8 + e] * lrn_exp2(-beta * lrn_log2(norm));
    }
    *reinterpret_cast<uint4 *>(y + pix * C + c0) = pack8(out);
  }
}

// Register/shuffle forms: a wave holds floor(64/tpp) whole pixels, tpp = C/8 lanes
// each with 8 channels; the cross-channel window's halo (<= 4 channels per side)
// comes from the neighbouring lanes by ds_bpermute (__shfl), so there is no LDS
// staging and no bank conflicts.  Every lane of the wave executes the shuffles.
struct LrnLane {
  long pix;
  int cv, tpp;
  bool active;
};
__device__ __forceinline__ LrnLane lrn_lane(long npix, int C) {
  LrnLane r;
  r.tpp = C / 8;
  const int ppw = 64 / r.tpp;  // whole pixels per wave
  const int lane = threadIdx.x & 63;
  const long wave = (static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int pl = lane / r.tpp;
  r.cv = lane - pl * r.tpp;
  r.pix = wave * ppw + pl;
  r.active = pl < ppw && r.pix < npix;
  return r;
}
// window sum over channels c-h..c+h of v (8 per lane), halo from neighbours
template <int H>
__device__ __forceinline__ void lrn_window_sum(const float *v, const LrnLane &L, float *out) {
  const int lane = threadIdx.x & 63;
  float lo[4], hi[4];  // lo[j] = channel c0-1-j (left lane), hi[j] = channel c0+8+j (right lane)
#pragma unroll
  for (int j = 0; j < H; ++j) {
    const float l = __shfl(v[7 - j], lane - 1);
    const float r = __shfl(v[j], lane + 1);
    lo[j] = L.cv > 0 ? l : 0.f;
    hi[j] = L.cv < L.tpp - 1 ? r : 0.f;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float s = 0.f;
#pragma unroll
    for (int d = -H; d <= H; ++d) {
      const int q = e + d;
      s += q < 0 ? lo[-q - 1] : (q > 7 ? hi[q - 8] : v[q]);
    }
    out[e] = s;
  }
}

// grid-stride over (4 waves x whole pixels) groups, at most 4096 blocks: on GoogLeNet's norm2
// (12.8M lanes) 60.5 -> 56.5 us against one-shot blocks.  (The gather-heavy fused pool -> LRN
// forward measured the other way, 78.7 -> 81.8 us on AlexNet, and keeps one-shot blocks.)
template <int H>
__global__ void __launch_bounds__(NT)
lrn_fwd_shfl(const bf16_t *__restrict__ x, bf16_t *__restrict__ y, long npix, int C, float salpha, float beta,
             float knorm, long ngroups) {
  LrnLane L;
  L.tpp = C / 8;
  const int ppw = 64 / L.tpp;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pl = lane / L.tpp;
  L.cv = lane - pl * L.tpp;
  for (long gi = blockIdx.x; gi < ngroups; gi += gridDim.x) {  // block-uniform: every lane shuffles
    L.pix = (gi * (NT / 64) + wave) * ppw + pl;
    L.active = pl < ppw && L.pix < npix;
    const long off = L.pix * C + L.cv * 8;
    float xv[8], sq[8], s[8];
    if (L.active) unpack8(*reinterpret_cast<const uint4 *>(x + off), xv);
    else
#pragma unroll
      for (int e = 0; e < 8; ++e) xv[e] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) sq[e] = xv[e] * xv[e];
    lrn_window_sum<H>(sq, L, s);
    if (!L.active) continue;
    float out[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = xv[e] * lrn_exp2(-beta * lrn_log2(knorm + salpha * s[e]));
    *reinterpret_cast<uint4 *>(y + off) = pack8(out);
  }
}
}  // namespace

// Launch shape of the shuffle forms: groups of NT / 64 waves, each wave holding 64 / (C / 8) whole
// pixels; sa = alpha / local_size.  A grid-stride kernel runs min(ngroups, cap) blocks.
struct LrnShfl {
  long ngroups;
  float sa;
  int blocks() const { return static_cast<int>(ngroups); }
  int blocks(long cap) const { return static_cast<int>(std::min<long>(ngroups, cap)); }
};
static inline LrnShfl lrn_shfl(long npix, int C, int nsize, float alpha) {
  const int tpp = C / 8;
  const long waves = (npix + 64 / tpp - 1) / (64 / tpp);
  return {(waves + NT / 64 - 1) / (NT / 64), alpha / nsize};
}

CXN_API int cxn_lrn_fwd(const void *x, void *y, long npix, int C, int nsize, float alpha, float beta, float knorm,
                        void *stream) {
  if (C % 8 != 0 || nsize / 2 > 4) return -1;
  if (C / 8 <= 64) {  // shuffle form
    const LrnShfl g = lrn_shfl(npix, C, nsize, alpha);
    with_half(nsize / 2, [&](auto hv) {
      CXN_LAUNCH((lrn_fwd_shfl<decltype(hv)::value>), g.blocks(4096), NT, 0, S_, (const bf16_t *)x, (bf16_t *)y, npix, C,
                 g.sa, beta, knorm, g.ngroups);
    });
    RET;
  }
  CXN_LAUNCH((lrn_fwd), nblocks(npix * C / 8), NT, 0, S_, (const bf16_t *)x, (bf16_t *)y, npix, C, nsize / 2, alpha / nsize,
                                                 beta, knorm);
  RET;
}

namespace {
// g_in[c] = g[c] norm[c]^-b - 2 b salpha x[c] sum_{c' in win(c)} g[c'] x[c'] norm[c']^(-b-1)
// (norm recomputed from x: no state tensor is stored)
// LDS-staged LRN backward: block = NT/(C/8) pixels, one thread per 8 channels.
// LDS per pixel: x, g and t = g*x*norm^(-b-1), each with `half` zero pads at both ends.
// mask_relu: the input is relu(z) of a fused producer -> also apply relu'(z) = (x > 0).
__global__ void lrn_bwd_lds(const bf16_t *x, const bf16_t *dy, bf16_t *dx, long npix, int C, int half, float salpha,
                            float beta, float knorm, int mask_relu) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tpp = C / 8;
  const int ppb = blockDim.x / tpp;
  const int L = C + 2 * half;
  const int pl = threadIdx.x / tpp, cv = threadIdx.x % tpp;
  const long pix = static_cast<long>(blockIdx.x) * ppb + pl;
  const bool active = pl < ppb && pix < npix;
  float *xs = sm + pl * 3 * L;
  float *gs = xs + L;
  float *ts = gs + L;
  const int c0 = cv * 8;
  float xv[8], gv[8];
  if (active) {
    unpack8(*reinterpret_cast<const uint4 *>(x + pix * C + c0), xv);
    unpack8(*reinterpret_cast<const uint4 *>(dy + pix * C + c0), gv);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      xs[half + c0 + e] = xv[e];
      gs[half + c0 + e] = gv[e];
    }
    if (cv == 0)
      for (int h = 0; h < half; ++h) {
        xs[h] = 0.f; xs[half + C + h] = 0.f;
        ts[h] = 0.f; ts[half + C + h] = 0.f;
      }
  }
  __syncthreads();
  float ng[8];
  if (active) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = half + c0 + e;
      float s = 0.f;
      for (int d = -half; d <= half; ++d) {
        const float v = xs[c + d];
        s += v * v;
      }
      const float lg = lrn_log2(knorm + salpha * s);
      const float p = lrn_exp2(-beta * lg);         // norm^-b
      ng[e] = gv[e] * p;
      ts[c] = gv[e] * xv[e] * p * lrn_exp2(-lg);    // g x norm^(-b-1)
    }
  }
  __syncthreads();
  if (active) {
    float out[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = half + c0 + e;
      float s = 0.f;
      for (int d = -half; d <= half; ++d) s += ts[c + d];
      out[e] = ng[e] - 2.f * beta * salpha * xv[e] * s;
      if (mask_relu && !(xv[e] > 0.f)) out[e] = 0.f;
    }
    *reinterpret_cast<uint4 *>(dx + pix * C + c0) = pack8(out);
  }
}

// dx may alias x (each lane reads its x/g before any write; the halo comes by shuffle).
template <int H>
__global__ void lrn_bwd_shfl(const bf16_t *x, const bf16_t *__restrict__ dy, bf16_t *dx, long npix, int C,
                             float salpha, float beta, float knorm, int mask_relu) {
  const LrnLane L = lrn_lane(npix, C);
  const long off = L.pix * C + L.cv * 8;
  float xv[8], gv[8], sq[8], s[8];
  if (L.active) {
    unpack8(*reinterpret_cast<const uint4 *>(x + off), xv);
    unpack8(*reinterpret_cast<const uint4 *>(dy + off), gv);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) xv[e] = gv[e] = 0.f;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) sq[e] = xv[e] * xv[e];
  lrn_window_sum<H>(sq, L, s);
  float ng[8], t[8], ts[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float lg = lrn_log2(knorm + salpha * s[e]);
    const float p = lrn_exp2(-beta * lg);  // norm^-b
    ng[e] = gv[e] * p;
    t[e] = gv[e] * xv[e] * p * lrn_exp2(-lg);  // g x norm^(-b-1)
  }
  lrn_window_sum<H>(t, L, ts);
  if (!L.active) return;
  float out[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    out[e] = ng[e] - 2.f * beta * salpha * xv[e] * ts[e];
    if (mask_relu && !(xv[e] > 0.f)) out[e] = 0.f;
  }
  *reinterpret_cast<uint4 *>(dx + off) = pack8(out);
}

__global__ void lrn_bwd(const bf16_t *__restrict__ x, const bf16_t *__restrict__ dy, bf16_t *__restrict__ dx,
                        long npix, int C, int half, float salpha, float beta, float knorm, int mask_relu) {
  const int CV = C / 8;
  const long total = npix * CV;
  for (long idx = grid_stride_start(); idx < total; idx += grid_stride()) {
    const long pix = idx / CV;
    const int c0 = (idx % CV) * 8;
    float xb[24], gb[24];
    load_window(x + pix * C, C, c0, xb);
    load_window(dy + pix * C, C, c0, gb);
    // t[j] = g x norm^(-b-1) for channels c0-8+j, j in [8-half, 16+half)
    float normv[24], tv[24];
#pragma unroll
    for (int j = 0; j < 24; ++j) {
      normv[j] = 1.f;
      tv[j] = 0.f;
    }
    for (int j = 8 - half; j < 16 + half; ++j) {
      float s = 0.f;
      for (int d = -half; d <= half; ++d) {
        const int q = j + d;
        const float v = (q >= 0 && q < 24) ? xb[q] : 0.f;
        s += v * v;
      }
      const float norm = knorm + salpha * s;
      normv[j] = norm;
      tv[j] = gb[j] * xb[j] * lrn_exp2((-beta - 1.f) * lrn_log2(norm));
    }
    float out[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int j = 8 + e;
      float s = 0.f;
      for (int d = -half; d <= half; ++d) s += tv[j + d];
      out[e] = gb[j] * lrn_exp2(-beta * lrn_log2(normv[j])) - 2.f * beta * salpha * xb[j] * s;
      if (mask_relu && !(xb[j] > 0.f)) out[e] = 0.f;
    }
    *reinterpret_cast<uint4 *>(dx + pix * C + c0) = pack8(out);
  }
}
}  // namespace

CXN_API int cxn_lrn_bwd(const void *x, const void *dy, void *dx, long npix, int C, int nsize, float alpha, float beta,
                        float knorm, int mask_relu, void *stream) {
  if (C % 8 != 0) return -1;
  const int half = nsize / 2;
  const int tpp = C / 8;  // threads per pixel
  if (tpp <= 64 && half <= 4) {  // shuffle form: whole pixels per wave
    const LrnShfl g = lrn_shfl(npix, C, nsize, alpha);
    with_half(half, [&](auto hv) {
      CXN_LAUNCH((lrn_bwd_shfl<decltype(hv)::value>), g.blocks(), NT, 0, S_, (const bf16_t *)x, (const bf16_t *)dy,
                 (bf16_t *)dx, npix, C, g.sa, beta, knorm, mask_relu);
    });
    RET;
  }
  if (tpp <= NT && (C + 2 * half) * 3 * 4 * (NT / tpp) <= 48 * 1024) {
    // LDS-staged form: each pixel row is read once, norm computed once per channel,
    // and dx may alias x (all reads of a pixel complete before its first write).
    const int ppb = NT / tpp;
    const int blocks = static_cast<int>((npix + ppb - 1) / ppb);
    const size_t smem = static_cast<size_t>(ppb) * (C + 2 * half) * 3 * sizeof(float);
    CXN_LAUNCH((lrn_bwd_lds), blocks, NT, smem, S_, (const bf16_t *)x, (const bf16_t *)dy, (bf16_t *)dx, npix, C, half,
                                          alpha / nsize, beta, knorm, mask_relu);
    RET;
  }
  if (half > 4 || x == dx) return -1;
  CXN_LAUNCH((lrn_bwd), nblocks(npix * C / 8), NT, 0, S_, (const bf16_t *)x, (const bf16_t *)dy, (bf16_t *)dx, npix, C,
                                                 half, alpha / nsize, beta, knorm, mask_relu);
  RET;
}

namespace {
// lrn_bwd_shfl plus the bias gradient of the conv in front (GoogLeNet conv2 -> relu -> norm2: the
// LRN's input gradient is that conv's output gradient): a grid-stride walk over the same
// (4 waves x whole pixels) groups, each lane summing the bf16 values it stores; the block's lanes
// meet in LDS in a fixed order and add one value per channel to db (not used in deterministic mode).
template <int H>
__global__ void __launch_bounds__(NT)
lrn_bwd_db(const bf16_t *x, const bf16_t *__restrict__ dy, bf16_t *dx, long npix, int C, float salpha, float beta,
           float knorm, int mask_relu, long ngroups, float *__restrict__ db, float *__restrict__ part) {
  __shared__ float red[NT * 8];
  LrnLane L;
  L.tpp = C / 8;
  const int ppw = 64 / L.tpp;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pl = lane / L.tpp;
  L.cv = lane - pl * L.tpp;
  float bs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bs[e] = 0.f;
  for (long gi = blockIdx.x; gi < ngroups; gi += gridDim.x) {  // block-uniform: every lane shuffles
    L.pix = (gi * (NT / 64) + wave) * ppw + pl;
    L.active = pl < ppw && L.pix < npix;
    const long off = L.pix * C + L.cv * 8;
    float xv[8], gv[8], sq[8], sw[8];
    if (L.active) {
      unpack8(*reinterpret_cast<const uint4 *>(x + off), xv);
      unpack8(*reinterpret_cast<const uint4 *>(dy + off), gv);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) xv[e] = gv[e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) sq[e] = xv[e] * xv[e];
    lrn_window_sum<H>(sq, L, sw);
    float ng[8], t[8], ts[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float lg = lrn_log2(knorm + salpha * sw[e]);
      const float pw = lrn_exp2(-beta * lg);
      ng[e] = gv[e] * pw;
      t[e] = gv[e] * xv[e] * pw * lrn_exp2(-lg);
    }
    lrn_window_sum<H>(t, L, ts);
    if (!L.active) continue;
    float out[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      out[e] = ng[e] - 2.f * beta * salpha * xv[e] * ts[e];
      if (mask_relu && !(xv[e] > 0.f)) out[e] = 0.f;
    }
    const uint4 pk = pack8(out);
    *reinterpret_cast<uint4 *>(dx + off) = pk;
    unpack8(pk, out);
#pragma unroll
    for (int e = 0; e < 8; ++e) bs[e] += out[e];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[threadIdx.x * 8 + e] = bs[e];
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += NT) {
    const int cv = c >> 3, e = c & 7;
    float s = 0.f;
    for (int w = 0; w < NT / 64; ++w)
      for (int p = 0; p < ppw; ++p) s += red[(w * 64 + p * L.tpp + cv) * 8 + e];
    if (part != nullptr) part[static_cast<long>(blockIdx.x) * C + c] = s;  // summed by part_rows_colsum
    else atomicAdd(db + c, s);
  }
}

// db[c] += sum_r part[r][c] over nrows fp32 partial rows of C columns: 32 columns x 8 row groups
// per block over a chunk of `chunk` rows (32: four dependent loads per thread, a few-us kernel
// instead of 11 us at 256), one atomic per column per chunk (one chunk: a fixed
// summation order, the deterministic mode)
__global__ void part_rows_colsum(const float *__restrict__ part, int nrows, int C, float *__restrict__ db, int chunk) {
  const int c = blockIdx.x * 32 + (threadIdx.x & 31);
  const int rg = threadIdx.x >> 5;
  const int r0 = blockIdx.y * chunk, r1 = min(nrows, r0 + chunk);
  float acc = 0.f;
  if (c < C)
    for (int r = r0 + rg; r < r1; r += 8) acc += part[static_cast<long>(r) * C + c];
  __shared__ float red[8][33];
  red[rg][threadIdx.x & 31] = acc;
  __syncthreads();
  if (rg == 0 && c < C) {
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) t += red[q][threadIdx.x & 31];
    atomicAdd(db + c, t);
  }
}
}  // namespace

// LRN backward plus db += the column sums of the stored dx (lrn_bwd_db): the shuffle form's
// shapes (C % 8 == 0, C / 8 <= 64, local_size <= 9); -1 otherwise (nothing launched).  part (fp32,
// part_floats >= 4096 * C): up to 4096 blocks store per-block sums there and part_rows_colsum
// adds them up; without it 1024 blocks add theirs with one atomic each per channel.
CXN_API int cxn_lrn_bwd_db(const void *x, const void *dy, void *dx, long npix, int C, int nsize, float alpha,
                           float beta, float knorm, int mask_relu, float *db, float *part, long part_floats,
                           void *stream) {
  if (C % 8 != 0 || C / 8 > 64 || nsize / 2 > 4 || db == nullptr || npix <= 0) return -1;
  const LrnShfl g = lrn_shfl(npix, C, nsize, alpha);
  if (part != nullptr && part_floats < 4096L * C) part = nullptr;
  const int blocks = g.blocks(part != nullptr ? 4096 : 1024);
  with_half(nsize / 2, [&](auto hv) {
    CXN_LAUNCH((lrn_bwd_db<decltype(hv)::value>), blocks, NT, 0, S_, (const bf16_t *)x, (const bf16_t *)dy, (bf16_t *)dx,
               npix, C, g.sa, beta, knorm, mask_relu, g.ngroups, db, part);
  });
  if (part != nullptr)
    CXN_LAUNCH((part_rows_colsum), dim3((C + 31) / 32, (blocks + 31) / 32), NT, 0, S_, part, blocks, C, db, 32);
  RET;
}

namespace {
// ------------------------------------------------------------------ fused max-pool -> LRN
// AlexNet's pool1 -> lrn1 and pool2 -> lrn2 (reference pooling_layer-inl.hpp:45-86 and
// lrn_layer-inl.hpp:53-74) as one kernel per direction.  Lanes are laid out as the shuffle LRN
// (whole pooled pixels per wave, C / 8 lanes each), so the cross-channel window sums stay in
// registers.
//   forward : the 3x3 / 2 max window (first max, offset byte, relu' bit as pool_fwd_rows) ->
//             pooled P and the LRN output Y in one pass: P is written (the LRN backward reads it)
//             but not read back;
//   backward: a block owns a band of R cell rows (2x2 input cells, pool_bwd_s2k3's
//             formulation) of one image.  Phase 1 computes the LRN data-gradient of the band's
//             windows (plus the row above, recomputed) from (P, dY) into LDS, masked by relu'
//             (bit 7 of the offset) and rounded to bf16 as the separate layers store it; phase 2
//             routes it from LDS to each cell's four pixels: the pooled gradient never reaches
//             HBM.  With dbias the conv-bias gradient behind a relu'd pool (the _fuse_pool_bias
//             sum of the pooled gradient) is summed over the band's own windows; per-block
//             partial rows in a fixed order.
// NN: the input is known to be >= 0 (a relu output: relu fused into the producing conv).  Then
// bf16 bits order as unsigned integers, and the first max of a window is one v_max_u32 per
// element over keys (bits << 16 | 15 - tap) -- the larger key is the larger value, then the
// earlier tap -- instead of unpack + compare + two selects.  The sign bit is cleared first: a
// relu of -0 may have stored -0 (0x8000), which must rank as 0.
template <int H, bool NN>
__global__ void pool_lrn_fwd(const bf16_t *__restrict__ x, bf16_t *__restrict__ P, uint8_t *__restrict__ arg,
                             bf16_t *__restrict__ Y, int N, int Hin, int Win, int C, int Ho, int Wo, int relu,
                             float salpha, float beta, float knorm) {
  const long npix = static_cast<long>(N) * Ho * Wo;
  const LrnLane L = lrn_lane(npix, C);
  float pv[8];
  uint32_t am[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    pv[q] = 0.f;
    am[q] = 0;
  }
  long o = 0;
  if (L.active) {
    const int n = static_cast<int>(L.pix / (static_cast<long>(Ho) * Wo));
    const int rem = static_cast<int>(L.pix - static_cast<long>(n) * Ho * Wo);
    const int ho = rem / Wo, wo = rem - (rem / Wo) * Wo;
    const int hs = 2 * ho, ws = 2 * wo;
    const bf16_t *xb = x + static_cast<long>(n) * Hin * Win * C + L.cv * 8;
    uint4 raw[9];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int h = min(hs + kh, Hin - 1), w = min(ws + kw, Win - 1);
        raw[kh * 3 + kw] = *reinterpret_cast<const uint4 *>(xb + (static_cast<long>(h) * Win + w) * C);
      }
    if constexpr (NN) {
      uint32_t best[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) best[q] = 0u;  // below every real key (>= 7)
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          if (hs + kh >= Hin || ws + kw >= Win) continue;
          const uint32_t t = 15u - static_cast<uint32_t>(kh * 3 + kw);
          const uint4 r = raw[kh * 3 + kw];
          const uint32_t wd[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            best[2 * q] = max(best[2 * q], ((wd[q] << 16) & 0x7fff0000u) | t);
            best[2 * q + 1] = max(best[2 * q + 1], (wd[q] & 0x7fff0000u) | t);
          }
        }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        pv[q] = __uint_as_float(best[q] & 0x7fff0000u);
        am[q] = 15u - (best[q] & 15u);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) pv[q] = -INFINITY;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          if (hs + kh >= Hin || ws + kw >= Win) continue;
          float v[8];
          unpack8(raw[kh * 3 + kw], v);
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const float a = (relu & 1) ? fmaxf(v[q], 0.f) : v[q];
            if (a > pv[q]) {
              pv[q] = a;
              am[q] = static_cast<uint32_t>(kh * 3 + kw);
            }
          }
        }
    }
    if (relu & 2)
#pragma unroll
      for (int q = 0; q < 8; ++q) am[q] |= pv[q] > 0.f ? 0u : 0x80u;
    o = L.pix * C + L.cv * 8;
    const uint4 pk = pack8(pv);
    *reinterpret_cast<uint4 *>(P + o) = pk;
    *reinterpret_cast<uint2 *>(arg + o) =
        make_uint2(am[0] | am[1] << 8 | am[2] << 16 | am[3] << 24, am[4] | am[5] << 8 | am[6] << 16 | am[7] << 24);
    unpack8(pk, pv);  // the LRN reads the stored (bf16) P, as the separate kernel would
  }
  float sq[8], sw[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) sq[e] = pv[e] * pv[e];
  lrn_window_sum<H>(sq, L, sw);
  if (!L.active) return;
  float out[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) out[e] = pv[e] * lrn_exp2(-beta * lrn_log2(knorm + salpha * sw[e]));
  *reinterpret_cast<uint4 *>(Y + o) = pack8(out);
}

template <int H>
__global__ void __launch_bounds__(NT)
lrn_pool_bwd(const bf16_t *__restrict__ P, const bf16_t *__restrict__ dY, const uint8_t *__restrict__ arg,
             bf16_t *__restrict__ dx, int Hin, int Win, int C, int Ho, int Wo, int HC, int WC, int R, int nband,
             int relu_bit, float salpha, float beta, float knorm, float *__restrict__ dbias_part) {
  extern __shared__ __attribute__((aligned(16))) char plds[];
  const int tpp = C / 8, ppw = 64 / tpp;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pl = lane / tpp, cv = lane - pl * tpp;
  const bool lane_ok = pl < ppw;
  LrnLane L;  // lrn_window_sum's view: channel block cv of a pixel of tpp lanes
  L.tpp = tpp;
  L.cv = cv;
  L.pix = 0;
  L.active = lane_ok;
  const int n = blockIdx.x / nband, band = blockIdx.x - n * nband;
  const int c0 = band * R;                                            // first cell row
  const int h_lo = max(c0 - 1, 0), h_hi = min(c0 + R - 1, Ho - 1);    // window rows it reads
  const int nwin = (h_hi - h_lo + 1) * Wo;
  bf16_t *const gl = reinterpret_cast<bf16_t *>(plds);                          // [window][C] gradient
  uint8_t *const al = reinterpret_cast<uint8_t *>(plds + static_cast<size_t>(R + 1) * Wo * C * 2);  // offsets
  const int step = (NT / 64) * ppw;
  // per-image bases (64-bit once); offsets inside one image fit 32 bits (checked by the launcher)
  const long pimg = static_cast<long>(n) * Ho * Wo * C;
  const bf16_t *const Pn = P + pimg;
  const bf16_t *const dYn = dY + pimg;
  const uint8_t *const an = arg + pimg;
  bf16_t *const dxn = dx + static_cast<long>(n) * Hin * Win * C;
  float bsum[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) bsum[k] = 0.f;
  // phase 1: the LRN data-gradient of every window of the band (and of the row above it), masked
  // by relu', rounded to bf16 as the separate layers store it, into LDS with the offsets
  // (window row, column) of this lane's window, advanced by `step` windows per pass (no divides)
  int wr = (wave * ppw + pl) / Wo, wc = (wave * ppw + pl) - wr * Wo;
  for (int base = 0; base < nwin; base += step) {
    const int wi = base + wave * ppw + pl;
    const bool ok = lane_ok && wi < nwin;
    const int ho = h_lo + wr, wo = wc;
    wc += step;
    while (wc >= Wo) {
      wc -= Wo;
      ++wr;
    }
    float xv[8], gv[8];
    uint2 a = make_uint2(0u, 0u);
    if (ok) {
      const int o = (ho * Wo + wo) * C + cv * 8;
      unpack8(*reinterpret_cast<const uint4 *>(Pn + o), xv);
      unpack8(*reinterpret_cast<const uint4 *>(dYn + o), gv);
      a = *reinterpret_cast<const uint2 *>(an + o);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) xv[e] = gv[e] = 0.f;
    }
    float sq[8], sw[8], t[8], ts[8], ng[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) sq[e] = xv[e] * xv[e];
    lrn_window_sum<H>(sq, L, sw);
#pragma unroll
    for (int e = 0; e < 8; ++e) {  // as lrn_bwd_shfl
      const float lg = lrn_log2(knorm + salpha * sw[e]);
      const float pw = lrn_exp2(-beta * lg);
      ng[e] = gv[e] * pw;
      t[e] = gv[e] * xv[e] * pw * lrn_exp2(-lg);
    }
    lrn_window_sum<H>(t, L, ts);
    if (!ok) continue;
    float gp[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) gp[e] = ng[e] - 2.f * beta * salpha * xv[e] * ts[e];
    unpack8(pack8(gp), gp);
    const uint32_t ab[8] = {a.x & 0xff, (a.x >> 8) & 0xff, (a.x >> 16) & 0xff, a.x >> 24,
                            a.y & 0xff, (a.y >> 8) & 0xff, (a.y >> 16) & 0xff, a.y >> 24};
#pragma unroll
    for (int e = 0; e < 8; ++e) gp[e] = (relu_bit && (ab[e] & 0x80u)) ? 0.f : gp[e];
    if (ho >= c0)  // rows c0.. are this band's own windows (row c0 - 1 belongs to the band above)
#pragma unroll
      for (int e = 0; e < 8; ++e) bsum[e] += gp[e];
    *reinterpret_cast<uint4 *>(gl + static_cast<long>(wi) * C + cv * 8) = pack8(gp);
    *reinterpret_cast<uint2 *>(al + static_cast<long>(wi) * C + cv * 8) =
        make_uint2(a.x & 0x7f7f7f7fu, a.y & 0x7f7f7f7fu);
  }
  __syncthreads();
  // phase 2: per 2x2 input cell the four windows that cover it (pool_bwd_s2k3's formulation)
  const int ncell = (min(c0 + R, HC) - c0) * WC;
  int cr = (wave * ppw + pl) / WC, cc = (wave * ppw + pl) - cr * WC;
  for (int base = 0; base < ncell; base += step) {
    const int ce = base + wave * ppw + pl;
    const int ci = c0 + cr, cj = cc;
    cc += step;
    while (cc >= WC) {
      cc -= WC;
      ++cr;
    }
    if (!lane_ok || ce >= ncell) continue;
    uint4 g[4];
    uint2 a[4];
    bool okw[4];
#pragma unroll
    for (int pq = 0; pq < 4; ++pq) {
      const int ho = ci - 1 + (pq >> 1), wo = cj - 1 + (pq & 1);
      okw[pq] = ho >= 0 && ho < Ho && wo >= 0 && wo < Wo;
      const int wi = okw[pq] ? (ho - h_lo) * Wo + wo : 0;
      g[pq] = *reinterpret_cast<const uint4 *>(gl + static_cast<long>(wi) * C + cv * 8);
      a[pq] = *reinterpret_cast<const uint2 *>(al + static_cast<long>(wi) * C + cv * 8);
    }
#pragma unroll
    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
      for (int sx = 0; sx < 2; ++sx) {
        const int h = 2 * ci + rr, w = 2 * cj + sx;
        if (h >= Hin || w >= Win) continue;
        float out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) out[k] = 0.f;
#pragma unroll
        for (int pq = 0; pq < 4; ++pq) {
          const int kh = 2 + rr - 2 * (pq >> 1), kw = 2 + sx - 2 * (pq & 1);  // tap of (h, w) in the window
          if (kh > 2 || kw > 2 || !okw[pq]) continue;
          const uint32_t off = static_cast<uint32_t>(kh * 3 + kw);
          float gv[8];
          unpack8(g[pq], gv);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            out[k] += ((a[pq].x >> (8 * k)) & 0xff) == off ? gv[k] : 0.f;
            out[k + 4] += ((a[pq].y >> (8 * k)) & 0xff) == off ? gv[k + 4] : 0.f;
          }
        }
        *reinterpret_cast<uint4 *>(dxn + (h * Win + w) * C + cv * 8) = pack8(out);
      }
  }
  if (dbias_part != nullptr) {  // the block's column sums in a fixed order (wave, pixel): no atomics
    // (in the window buffer, done with after phase 2: no extra LDS, so no lower occupancy)
    __syncthreads();
    float(*red)[64][9] = reinterpret_cast<float(*)[64][9]>(plds);
#pragma unroll
    for (int k = 0; k < 8; ++k) red[wave][lane][k] = lane_ok ? bsum[k] : 0.f;
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      const int cc = c >> 3, k = c & 7;
      float acc = 0.f;
      for (int w = 0; w < NT / 64; ++w)
        for (int j = 0; j < ppw; ++j) acc += red[w][j * tpp + cc][k];
      dbias_part[static_cast<long>(blockIdx.x) * C + c] = acc;
    }
  }
}
}  // namespace

// the fused pair serves a ceil-mode 3x3 / 2 max pool without padding in front of a shuffle-form LRN
static inline bool pool_lrn_served(int Hin, int Win, int C, int Ho, int Wo, int nsize) {
  if (C % 8 || C / 8 > 64 || nsize / 2 > 4 || Hin < 3 || Win < 3) return false;
  return Ho == min(Hin - 2, Hin - 1) / 2 + 1 && Wo == min(Win - 2, Win - 1) / 2 + 1;
}

// fused max-pool (3x3 / 2, pad 0) -> LRN; see pool_lrn_fwd / lrn_pool_bwd.  -1: not served.
CXN_API int cxn_pool_lrn_fwd(const void *x, void *P, void *arg, void *Y, int N, int Hin, int Win, int C, int Ho, int Wo,
                             int relu, int nsize, float alpha, float beta, float knorm, void *stream) {
  if (!pool_lrn_served(Hin, Win, C, Ho, Wo, nsize)) return -1;
  const LrnShfl g = lrn_shfl(static_cast<long>(N) * Ho * Wo, C, nsize, alpha);
  // relu bit 2 (4): the input is a relu output (>= 0): the integer-key max (pool_lrn_fwd NN)
  const bool nn = (relu & 4) != 0 && (relu & 1) == 0;
  with_half(nsize / 2, [&](auto hv) {
    with_flag(nn, [&](auto nnv) {
      CXN_LAUNCH((pool_lrn_fwd<decltype(hv)::value, decltype(nnv)::value>), g.blocks(), NT, 0, S_, (const bf16_t *)x,
                 (bf16_t *)P, (uint8_t *)arg, (bf16_t *)Y, N, Hin, Win, C, Ho, Wo, relu, g.sa, beta, knorm);
    });
  });
  RET;
}
// dbias_part: fp32 [blocks][C] per-block partial sums of the masked pooled gradient (null: no
// bias sum); part_rows < 0: only return the block count.  Returns the block count (>= 0), -1
// when not served, -4 when part_rows is too small.  det: the partial rows summed in one fixed
// order (else 256-row chunks added atomically).
CXN_API int cxn_lrn_pool_bwd(const void *P, const void *dY, const void *arg, void *dx, int N, int Hin, int Win, int C,
                             int Ho, int Wo, int relu_bit, int nsize, float alpha, float beta, float knorm,
                             float *dbias, float *dbias_part, long part_rows, int det, void *stream) {
  if (!pool_lrn_served(Hin, Win, C, Ho, Wo, nsize) || N < 1) return -1;
  const int HC = (Hin + 1) / 2, WC = (Win + 1) / 2;
  // cell rows per block: the band's windows (R + 1 rows: one row recomputed) staged in LDS as bf16
  // gradient + offset byte, within 56 KiB of dynamic LDS (the bias partials take 9 KiB more)
  const long row_bytes = static_cast<long>(Wo) * C * 3;
  static const int r_env = [] {  // CXN_LRN_POOL_R: probe override of the band height
    const char *e = std::getenv("CXN_LRN_POOL_R");
    return e != nullptr ? std::atoi(e) : 0;
  }();
  // 4 rows, 2 for wide-channel maps (AlexNet pool1 C = 96: R 4 70.4 us, R 2 77.1; pool2 C = 256:
  // R 4 56.8 us, R 2 51.0 -- profiles/r5_lrn_pool_bwd_band_probe.jsonl)
  int R = r_env > 0 ? r_env : (C >= 192 ? 2 : 4);
  while (R > 1 && (R + 1) * row_bytes > 56 * 1024) --R;
  if ((R + 1) * row_bytes > 56 * 1024) return -1;
  if (static_cast<long>(Hin) * Win * C >= (1L << 31)) return -1;  // 32-bit offsets inside an image
  const int nband = (HC + R - 1) / R;
  const long blocks_l = static_cast<long>(N) * nband;
  if (blocks_l >= (1L << 31)) return -1;
  const int blocks = static_cast<int>(blocks_l);
  if (part_rows < 0) return blocks;  // query
  const float sa = alpha / nsize;
  float *part = dbias != nullptr ? dbias_part : nullptr;
  if (dbias != nullptr && (part == nullptr || part_rows < blocks)) return -4;
  // (the bias partials reuse the window buffer: at least NT x 9 floats)
  const size_t lds = std::max(static_cast<size_t>((R + 1) * row_bytes), static_cast<size_t>(NT * 9 * 4));
  with_half(nsize / 2, [&](auto hv) {
    CXN_LAUNCH((lrn_pool_bwd<decltype(hv)::value>), blocks, NT, lds, S_, (const bf16_t *)P, (const bf16_t *)dY,
               (const uint8_t *)arg, (bf16_t *)dx, Hin, Win, C, Ho, Wo, HC, WC, R, nband, relu_bit, sa, beta, knorm, part);
  });
  if (part != nullptr) {
    const int chunk = det ? blocks : 32;  // 4 rows per thread: latency-bound otherwise
    CXN_LAUNCH((part_rows_colsum), dim3((C + 31) / 32, (blocks + chunk - 1) / chunk), NT, 0, S_, part, blocks, C,
               dbias, chunk);
  }
  if (hipGetLastError() != hipSuccess) return -3;
  return blocks;
}
