// GPU affine warp stage: the random rotate / shear / scale / aspect augmentation as one kernel
// over the batch (affine_gpu = 1, io/warp_stage.py).
//
// Reference behaviour: src/io/image_augmenter-inl.hpp:74-121 (cv::warpAffine, INTER_CUBIC,
// BORDER_CONSTANT, then the crop) and the mirror of src/io/iter_augment_proc-inl.hpp:98-162.
// The host (runtime/jpeg_decode.h DrawWarp / DecodeRegion) draws each record's augmentation,
// folds warp, crop and mirror into one output-pixel -> source-position map and decodes the
// part of the image the map can touch into a packed RGB buffer.  The arithmetic here is the
// published fixed-point scheme of that warp (1/32-pixel coordinates, bicubic A = -0.75,
// 15-bit weights, constant border), defined in integers by io/warp_stage.py warp_reference;
// the batch is bit-equal to it (tests/test_warp_stage_gpu.py).
//
// Layout: src uint8 packed regions (rw * rh * 3 bytes each, RGB), table int64 [B][16]
// (runtime/jpeg_decode.h WarpTableField), wtab int32 [32][32][16] (fy, fx, 4 x 4 taps).
#include "common.h"

namespace {

constexpr int kTable = 16, kValid = 0, kOffset = 1, kX0 = 2, kY0 = 3, kRw = 4, kRh = 5, kImgW = 6, kImgH = 7,
              kM0 = 8, kFill = 14;

struct Px12 {
  uint8_t v[12];
} __attribute__((packed, aligned(1)));

// round-half-even of a coordinate in 1/1024 pixel.  The product and the sum are separate
// correctly rounded operations on purpose: a fused m1 * y + m2 rounds once instead of twice and
// would differ from the float64 reference within an ulp of a half, which no test image shows.
// __dmul_rn / __dadd_rn are plain operators in this toolchain's headers (hipcc contracts them),
// so contraction is switched off for these two functions instead; the kernel's ISA has no
// v_fma_f64.
__device__ __forceinline__ int fix_mul(double m, int v) {
#pragma clang fp contract(off)
  const double p = m * static_cast<double>(v);
  return static_cast<int>(rint(p * 1024.0));
}
__device__ __forceinline__ int fix_mad(double m, int v, double c) {
#pragma clang fp contract(off)
  const double p = m * static_cast<double>(v);
  const double s = p + c;
  return static_cast<int>(rint(s * 1024.0));
}

// One thread per output pixel (all channels), 16 x 16 output tiles: a block's source footprint
// stays a compact patch under any rotation, so the 16 taps of neighbouring pixels come from cache.
// grid (cdiv(w, 16), cdiv(h, 16), rows)
__global__ void __launch_bounds__(256) image_warp(const uint8_t *__restrict__ src, const long long *__restrict__ table,
                                                  const int *__restrict__ wtab, int h, int w, int C,
                                                  uint8_t *__restrict__ out) {
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x >= w || y >= h) return;
  const long long *t = table + static_cast<long>(blockIdx.z) * kTable;
  uint8_t *o = out + ((static_cast<long>(blockIdx.z) * h + y) * w + x) * C;
  if (t[kValid] == 0) {  // padding row or another rank's row
    for (int k = 0; k < C; ++k) o[k] = 0;
    return;
  }
  const int x0 = static_cast<int>(t[kX0]), y0 = static_cast<int>(t[kY0]), rw = static_cast<int>(t[kRw]),
            rh = static_cast<int>(t[kRh]), W = static_cast<int>(t[kImgW]), H = static_cast<int>(t[kImgH]);
  const int fill = static_cast<int>(t[kFill]);
  const bool empty = rw <= 0 || rh <= 0;
  const uint8_t *reg = src + t[kOffset];  // 64-bit byte offset
  const int X = (fix_mad(__longlong_as_double(t[kM0 + 1]), y, __longlong_as_double(t[kM0 + 2])) + 16 +
                 fix_mul(__longlong_as_double(t[kM0]), x)) >> 5;
  const int Y = (fix_mad(__longlong_as_double(t[kM0 + 4]), y, __longlong_as_double(t[kM0 + 5])) + 16 +
                 fix_mul(__longlong_as_double(t[kM0 + 3]), x)) >> 5;
  const int ix = (X >> 5) - 1, iy = (Y >> 5) - 1;
  const int4 *wq = reinterpret_cast<const int4 *>(wtab + ((Y & 31) * 32 + (X & 31)) * 16);
  const int rx = ix - x0;
  // the four taps of a row are inside the image and the region: 12 contiguous bytes
  const bool row_fast = !empty && ix >= 0 && ix + 3 < W && rx >= 0 && rx + 3 < rw;
  int acc[3] = {0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int4 wv = wq[j];
    const int wt[4] = {wv.x, wv.y, wv.z, wv.w};
    const int sy = iy + j, ry = sy - y0;
    const bool in_y = sy >= 0 && sy < H;
    if (row_fast && in_y && ry >= 0 && ry < rh) {
      Px12 p;
      __builtin_memcpy(&p, reg + (static_cast<long>(ry) * rw + rx) * 3, 12);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] += static_cast<int>(p.v[i * 3 + k]) * wt[i];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int sx = ix + i;
        int v[3] = {fill, fill, fill};
        if (!empty && in_y && sx >= 0 && sx < W) {
          // a tap inside the image is inside the region by construction; the clamp keeps a
          // wrong table from reading outside the region
          const int cx = min(max(sx - x0, 0), rw - 1), cy = min(max(ry, 0), rh - 1);
          const uint8_t *p = reg + (static_cast<long>(cy) * rw + cx) * 3;
          v[0] = p[0], v[1] = p[1], v[2] = p[2];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] += v[k] * wt[i];
      }
    }
  }
  for (int k = 0; k < C; ++k) o[k] = static_cast<uint8_t>(min(max((acc[k] + 16384) >> 15, 0), 255));
}

}  // namespace


// src packed RGB regions, table int64 [B][16], wtab int32 [32][32][16] (16-byte aligned) ->
// out uint8 [r1 - r0][h][w][C] for batch rows r0..r1.  The caller checked the regions against the
// packed buffer (ops.image_warp).
CXN_API int cxn_image_warp(const void *src, const void *table, const void *wtab, int r0, int r1, int h, int w, int C,
                           void *out, void *stream) {
  if (C < 1 || C > 3 || r0 < 0 || r1 < r0 || h <= 0 || w <= 0 || r1 - r0 > 65535 || cdiv(h, 16) > 65535) return -2;
  if (reinterpret_cast<uintptr_t>(wtab) % 16 != 0 || reinterpret_cast<uintptr_t>(table) % 8 != 0) return -2;
  if (r1 == r0) return 0;
  CXN_LAUNCH((image_warp), dim3(cdiv(w, 16), cdiv(h, 16), r1 - r0), 256, 0, S_, (const uint8_t *)src,
             (const long long *)table + static_cast<long>(r0) * kTable, (const int *)wtab, h, w, C, (uint8_t *)out);
  RET;
}
