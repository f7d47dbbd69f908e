// The second launch of the depthwise weight gradients (dwconv_kernels.hip, dwconv_lk_kernels.hip):
// the fixed-order merge of the per-block fp32 slabs.  Included inside each file's anonymous
// namespace, after its NT (256).
#pragma once

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
