// loss layers and evaluation metrics on the device.
//
//   cxn_softmax       row softmax of bf16 scores into bf16 and, optionally, fp32 probabilities
//   cxn_loss_grad     (p - target) * scale in place over the node: softmax, l2, multi-logistic
//                     (reference loss/softmax_layer-inl.hpp)
//   cxn_metric_eval   error / logloss / rec@n sums of a batch added into a float64 accumulator
//                     (reference src/utils/metric.h:20-236)
//
// Return 0, -1 for more metrics than one launch serves, or -3 when a launch failed.
#include "nn_shared.h"

namespace {
// One wave per row.  p = softmax(x) written to y (bf16) and optionally pf (fp32).
__global__ void softmax_rows(const bf16_t *__restrict__ x, bf16_t *__restrict__ y, float *__restrict__ pf,
                             int rows, int K) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bf16_t *xr = x + static_cast<long>(row) * K;
  float m = -INFINITY;
  for (int k = lane; k < K; k += 64) m = fmaxf(m, bf2f(xr[k]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  float s = 0.f;
  for (int k = lane; k < K; k += 64) s += __expf(bf2f(xr[k]) - m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float inv = 1.f / s;
  for (int k = lane; k < K; k += 64) {
    const float p = __expf(bf2f(xr[k]) - m) * inv;
    y[static_cast<long>(row) * K + k] = f2bf(p);
    if (pf) pf[static_cast<long>(row) * K + k] = p;
  }
}

// Rows of K <= 64 * NPL: one wave per row, one block per row (every CU gets rows), the row held in
// registers -- all of its loads issued before the first reduction instead of three dependent
// passes over memory (AlexNet fc8 output, 256 x 1000: 9.1 -> a few us).  Same arithmetic as
// softmax_rows: max, sum of exp(x - max), one reciprocal.
template <int NPL>
__global__ void __launch_bounds__(64) softmax_rows_reg(const bf16_t *__restrict__ x, bf16_t *__restrict__ y,
                                                       float *__restrict__ pf, int K) {
  const int lane = threadIdx.x;
  const long base = static_cast<long>(blockIdx.x) * K;
  float v[NPL];
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    const int k = lane + 64 * j;
    v[j] = k < K ? bf2f(x[base + k]) : -INFINITY;
  }
  float m = v[0];
#pragma unroll
  for (int j = 1; j < NPL; ++j) m = fmaxf(m, v[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    v[j] = lane + 64 * j < K ? __expf(v[j] - m) : 0.f;
    s += v[j];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float inv = 1.f / s;
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    const int k = lane + 64 * j;
    if (k < K) {
      const float p = v[j] * inv;
      y[base + k] = f2bf(p);
      if (pf) pf[base + k] = p;
    }
  }
}
}  // namespace

CXN_API int cxn_softmax(const void *x, void *y, float *pf, int rows, int K, void *stream) {
  if (rows <= 0) return 0;
  if (K <= 1024 && rows < (1 << 30)) {
    const bf16_t *xb = (const bf16_t *)x;
    bf16_t *yb = (bf16_t *)y;
    if (K <= 256) CXN_LAUNCH((softmax_rows_reg<4>), rows, 64, 0, S_, xb, yb, pf, K);
    else if (K <= 512) CXN_LAUNCH((softmax_rows_reg<8>), rows, 64, 0, S_, xb, yb, pf, K);
    else CXN_LAUNCH((softmax_rows_reg<16>), rows, 64, 0, S_, xb, yb, pf, K);
    RET;
  }
  CXN_LAUNCH((softmax_rows), cdiv(rows, 4), 256, 0, S_, (const bf16_t *)x, (bf16_t *)y, pf, rows, K);
  RET;
}

namespace {
// grad = (p - onehot(label)) * scale, written in place over the bf16 node.  kind 0 softmax,
// 1 l2 (x - y), 2 multi-logistic (sigma - y, node already holds sigma).  label: fp32 [rows][lw]
__global__ void loss_grad(const float *__restrict__ p32, bf16_t *__restrict__ node, const float *__restrict__ label,
                          int rows, int K, int lw, float scale, int kind) {
  const long total = static_cast<long>(rows) * K;
  for (long i = grid_stride_start(); i < total; i += grid_stride()) {
    const int r = i / K, k = i % K;
    const float p = p32 ? p32[i] : bf2f(node[i]);
    float g;
    if (kind == 0) g = p - (static_cast<int>(label[static_cast<long>(r) * lw]) == k ? 1.f : 0.f);
    else g = p - label[static_cast<long>(r) * lw + k];
    node[i] = f2bf(g * scale);
  }
}
}  // namespace

CXN_API int cxn_loss_grad(const float *p32, void *node, const float *label, int rows, int K, int lw, float scale,
                          int kind, void *stream) {
  CXN_LAUNCH((loss_grad), nblocks(static_cast<long>(rows) * K), NT, 0, S_, p32, (bf16_t *)node, label, rows, K, lw, scale, kind);
  RET;
}

namespace {
// Training / eval metrics on the device (reference src/utils/metric.h:20-236), one wave per
// instance row of fp32 scores p[B][K] against labels lab[B][lw]:
//   kind 0 error   : first-max argmax != label[0]   (K == 1: score > 0 is class 1)
//   kind 1 logloss : -log(clamp(p[label[0]], 1e-15, 1 - 1e-15))   (K == 1: binary form)
//   kind 2 rec@n   : (#distinct labels ranked within the top n) / lw, where a label's rank
//                    counts the scores that are larger, or equal at a lower index (the
//                    reference breaks exact ties at random; here the lowest index ranks first,
//                    so at most n labels can hit).
// Each block writes the sums over its rows to part[block][metric]; metric_accum adds the
// block partials, in block order, into a float64 accumulator (deterministic, no atomics).
struct MetricSpec {
  int nm;
  int kind[8];
  int arg[8];
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(256) metric_rows(const float *__restrict__ p, int ldp, const float *__restrict__ lab,
                                                  int ldl, int lw, int B, int K, MetricSpec ms, float *__restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) acc[m] = 0.f;
  for (int r = blockIdx.x * 4 + wave; r < B; r += gridDim.x * 4) {
    const float *pr = p + static_cast<long>(r) * ldp;
    const float *lr = lab + static_cast<long>(r) * ldl;
    const int l0 = static_cast<int>(lr[0]);
    // first-max argmax
    float mv = -INFINITY;
    int mi = 0x7fffffff;
    for (int j = lane; j < K; j += 64) {
      const float v = pr[j];
      if (v > mv) { mv = v; mi = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(mv, o, 64);
      const int oi = __shfl_xor(mi, o, 64);
      if (ov > mv || (ov == mv && oi < mi)) { mv = ov; mi = oi; }
    }
    for (int m = 0; m < ms.nm; ++m) {
      float v = 0.f;
      if (ms.kind[m] == 0) {
        const int pred = K == 1 ? (pr[0] > 0.f ? 1 : 0) : mi;
        v = pred != l0 ? 1.f : 0.f;
      } else if (ms.kind[m] == 1) {
        if (K != 1) {
          const float q = fminf(fmaxf(pr[l0], 1e-15f), 1.f - 1e-15f);
          v = -logf(q);
        } else {
          const float py = fminf(fmaxf(pr[0], 1e-15f), 1.f - 1e-15f), y = lr[0];
          v = -(y * logf(py) + (1.f - y) * logf(1.f - py));
        }
      } else {
        const int n = ms.arg[m];
        int hits = 0;
        for (int c = 0; c < lw; ++c) {
          const int lc = static_cast<int>(lr[c]);
          bool dup = false;
          for (int d = 0; d < c; ++d) dup |= static_cast<int>(lr[d]) == lc;
          if (dup || lc < 0 || lc >= K) continue;
          const float sl = pr[lc];
          float cnt = 0.f;
          for (int j = lane; j < K; j += 64) cnt += (pr[j] > sl || (pr[j] == sl && j < lc)) ? 1.f : 0.f;
          cnt = wave_sum(cnt);
          hits += cnt < static_cast<float>(n) ? 1 : 0;
        }
        v = static_cast<float>(hits) / static_cast<float>(lw);
      }
      acc[m] += v;  // identical in every lane of the wave
    }
  }
  __shared__ float red[4][8];
  if (lane == 0)
#pragma unroll
    for (int m = 0; m < 8; ++m) red[wave][m] = acc[m];
  __syncthreads();
  if (threadIdx.x < ms.nm)
    part[blockIdx.x * ms.nm + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

__global__ void metric_accum(const float *__restrict__ part, int nb, int nm, double *__restrict__ acc) {
  const int m = threadIdx.x;
  if (m < nm) {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part[b * nm + m];
    acc[m] += s;
  }
}
}  // namespace

// acc: float64 [nm] metric sums (+= this batch); part: fp32 workspace of >= 256*nm floats.
CXN_API int cxn_metric_eval(const float *p, int ldp, const float *lab, int ldl, int lw, int B, int K, int nm,
                            const int *kinds, const int *args, double *acc, float *part, void *stream) {
  if (nm < 1 || nm > 8 || B < 1) return nm < 1 || B < 1 ? 0 : -1;
  MetricSpec ms{};
  ms.nm = nm;
  for (int m = 0; m < nm; ++m) {
    ms.kind[m] = kinds[m];
    ms.arg[m] = args[m];
  }
  int nb = (B + 3) / 4;
  if (nb > 256) nb = 256;
  CXN_LAUNCH((metric_rows), nb, 256, 0, S_, p, ldp, lab, ldl, lw, B, K, ms, part);
  CXN_LAUNCH((metric_accum), 1, 64, 0, S_, part, nb, nm, acc);
  RET;
}
